// obs.hip — k_obs: opponent masks and every observation tensor.
#include "sim_dev.h"

namespace mpenv {

__device__ __forceinline__ Vec3 normalizedPosD(const SceneDev &sc, Vec3 p) // sim.cpp:2693-2718
{
    float min_x = sc.worldBounds.pMin.x, min_y = sc.worldBounds.pMin.y, min_z = sc.worldBounds.pMin.z;
    float max_x = sc.worldBounds.pMax.x, max_y = sc.worldBounds.pMax.y, max_z = sc.worldBounds.pMax.z;
    float xr = max_x - min_x, yr = max_y - min_y, zr = max_z - min_z;
    float x = (p.x - min_x) / xr, y = (p.y - min_y) / yr, z = (p.z - min_z) / zr;
    return v3(clampf(x, 0.f, 1.f), clampf(y, 0.f, 1.f), clampf(z, 0.f, 1.f));
}

struct SelfFrame {
    Vec3 pos;
    Quat invRot;
    float yaw, pitch;
};

__device__ __forceinline__ void relAnglesD(const SelfFrame &sf, Vec3 to, float &dist_out, float &yaw_out,
                                           float &pitch_out)
{
    float d = length(to);
    if (d < 1e-2f) {
        dist_out = 0.f; yaw_out = 0.f; pitch_out = 0.f;
        return;
    }
    to = to / d;
    float new_yaw = -atan2f_(to.x, to.y);
    float new_pitch = asinf_(clampf(to.z, -1.f, 1.f));
    float yaw_delta = new_yaw - sf.yaw;
    float pitch_delta = new_pitch - sf.pitch;
    if (yaw_delta > kPi) yaw_delta -= 2.f * kPi;
    else if (yaw_delta < -kPi) yaw_delta += 2.f * kPi;
    dist_out = d; yaw_out = yaw_delta; pitch_out = pitch_delta;
}

__device__ __forceinline__ Vec3 normalizedPosUnclampedD(const SceneDev &sc, Vec3 p)
{
    float min_x = sc.worldBounds.pMin.x, min_y = sc.worldBounds.pMin.y, min_z = sc.worldBounds.pMin.z;
    float max_x = sc.worldBounds.pMax.x, max_y = sc.worldBounds.pMax.y, max_z = sc.worldBounds.pMax.z;
    float xr = max_x - min_x, yr = max_y - min_y, zr = max_z - min_z;
    return v3((p.x - min_x) / xr, (p.y - min_y) / yr, (p.z - min_z) / zr);
}

// ---- k_obs: pvpOpponentMasksSystem (sim.cpp:2562-2614), pvpObservationsSystem
// (sim.cpp:2645-3052) and fullTeamObservationsSystem (sim.cpp:3054-3301).
//
// Load first, then store.  gfx9's vector-memory counter retires loads and
// stores in issue order, so a load issued after a burst of stores cannot be
// waited for without waiting for those stores' write acknowledgements too.
// The round-1..4 k_obs gathered each world-mate's fields from HBM/L2 inside
// its slot loop, between the previous slot's row stores: every slot paid a
// full store round trip (55 `s_waitcnt vmcnt(0)` in its ISA; ~95 us per wave
// for ~141 KB of rows, 3.4 TB/s).  Now every input is read before the first
// store: a block (256 consecutive agents) stages the columns of every agent
// of its worlds in LDS (<= 256 + 2 (N - 1) agents, coalesced column loads),
// each lane loads its own rotation and world fields, and from then on the
// kernel only reads LDS and stores.
//
// Rows leave through a per-wave LDS transpose, half a wave (32 rows) at a
// time so the stage fits next to the agent columns (3 blocks per CU): a
// lane computes its row in registers, its half writes the rows to LDS, and
// every lane of the wave stores whole row pieces (float4 where the rows are
// 16-B aligned), so a store instruction writes a few whole 128-B lines
// instead of one 4-16 B piece of 64 different rows.
constexpr int kObsBlock = 256;
constexpr int kObsStageMax = kObsBlock + 2 * (kMaxAgents - 1); // the block's agents plus a partial world at each end
enum : int {
    kOsPX, kOsPY, kOsPZ, kOsVX, kOsVY, kOsVZ, kOsYaw, kOsPitch, kOsDYV, kOsDPV, kOsHP, kOsFired, kOsAlive, // f32
    kOsCurPose, kOsTgtPose, kOsWeapon, kOsVis, kOsTrans, kOsFlags, kOsShot, kOsHeal, kOsMag0, kOsMag1,      // i32
    kObsCols
};
constexpr int kObsRowPad = kOtherObs + 4; // LDS row stride (floats) of the 32-float rows: 16-B aligned
constexpr int kObsSpanPad = 44;           // floats per staged row: >= kObsRowPad and the 43-float self obs

// The block's agent columns in LDS (index = global agent id - s0).
struct ObsStage {
    const float (*c)[kObsStageMax];
    __device__ __forceinline__ float f(int col, int k) const { return c[col][k]; }
    __device__ __forceinline__ int32_t i(int col, int k) const { return __float_as_int(c[col][k]); }
    __device__ __forceinline__ Vec3 pos(int k) const { return v3(c[kOsPX][k], c[kOsPY][k], c[kOsPZ][k]); }
    __device__ __forceinline__ Vec3 vel(int k) const { return v3(c[kOsVX][k], c[kOsVY][k], c[kOsVZ][k]); }
    __device__ __forceinline__ bool alive(int k) const { return c[kOsAlive][k] != 0.f; }
};

// fillCommonOb (sim.cpp:2720-2774) of stage agent j into a register array;
// returns alive.
__device__ __forceinline__ bool fillCommonS(const ObsStage &st, const SceneDev &sc, const SelfFrame &sf, int j,
                                            float *ob, float *pos_ob)
{
    ob[0] = 1.f;
    if (!st.alive(j)) return false;
    ob[1] = 1.f;
    Vec3 np = normalizedPosD(sc, st.pos(j));
    ob[2] = np.x; ob[3] = np.y; ob[4] = np.z;
    pos_ob[0] = np.x; pos_ob[1] = np.y; pos_ob[2] = np.z;
    ob[5] = 0.5f * ((st.f(kOsYaw, j) / kPi) + 1.f);
    ob[6] = 0.5f * (st.f(kOsPitch, j) / (0.25f * kPi) + 1.f);
    Vec3 rv = rotateVec(sf.invRot, st.vel(j));
    ob[7] = rv.x; ob[8] = rv.y; ob[9] = rv.z;
    ob[10] = st.f(kOsDYV, j); ob[11] = st.f(kOsDPV, j);
    const int cp = st.i(kOsCurPose, j), tp = st.i(kOsTgtPose, j);
    ob[12] = cp == kStand ? 1.f : 0.f;
    ob[13] = cp == kCrouch ? 1.f : 0.f;
    ob[14] = cp == kProne ? 1.f : 0.f;
    ob[15] = tp == kStand ? 1.f : 0.f;
    ob[16] = tp == kCrouch ? 1.f : 0.f;
    ob[17] = tp == kProne ? 1.f : 0.f;
    ob[18] = (float)st.i(kOsTrans, j) / (float)c::kPoseTransitionSpeed;
    ob[19] = (st.i(kOsFlags, j) & kFlagInZone) ? 1.f : 0.f;
    const int wt = st.i(kOsWeapon, j);
    ob[20] = wt == 0 ? 1.f : 0.f;
    ob[21] = wt == 1 ? 1.f : 0.f;
    ob[22] = wt == 2 ? 1.f : 0.f;
    return true;
}

__device__ __forceinline__ void fillCombatS(const ObsStage &st, int j, float *ob)
{
    ob[0] = st.f(kOsHP, j) / 100.f;
    ob[1] = (float)st.i(kOsMag0, j);
    ob[2] = (float)st.i(kOsMag1, j);
    ob[3] = float(st.i(kOsHeal, j)) / float(c::kOutOfCombatSteps);
}

__device__ __forceinline__ void fillOtherS(const ObsStage &st, const SelfFrame &sf, int j, float *ob)
{
    relAnglesD(sf, st.pos(j) - sf.pos, ob[23], ob[24], ob[25]);
    float rfy = st.f(kOsYaw, j) - sf.yaw;
    float rfp = st.f(kOsPitch, j) - sf.pitch;
    if (rfy > kPi) rfy -= 2.f * kPi;
    else if (rfy < -kPi) rfy += 2.f * kPi;
    ob[26] = rfy;
    ob[27] = rfp;
}

// Half-wave row stage.  `buf` holds 32 rows (stride P <= kObsSpanPad floats)
// and `offs` 32 row offsets.  Half h = lanes [32h, 32h + 32) of the wave's
// m live lanes (a tail wave's lanes past A have returned).  Pattern:
//   stage(h, ...) by the half's lanes -> waveSync -> flush*(h, ...) by every
//   live lane -> waveSync (reads done before the next rows land).
// The cross-lane exchange stays inside one wave: the wave's DS instructions
// execute in issue order, so only the compiler needs ordering, which the
// wavefront-scope fences of waveSync give.
struct HalfStage {
    float *buf;
    int64_t *offs;
    int lane, m;

    __device__ __forceinline__ int halves() const { return m > 32 ? 2 : 1; }
    __device__ __forceinline__ int rowsOf(int h) const { return m - 32 * h < 32 ? m - 32 * h : 32; }
    __device__ __forceinline__ bool mine(int h) const { return (lane >> 5) == h; }
    template <int P> __device__ __forceinline__ void stage(int h, const float *v, int n, int at = 0) const
    {
        if (mine(h))
            for (int k = 0; k < n; k++) buf[(lane & 31) * P + at + k] = v[k];
    }
    __device__ __forceinline__ void stageOff(int h, int64_t off) const
    {
        if (mine(h)) offs[lane & 31] = off;
    }
    // Rows of half h back to back from dst (row r at dst + r * n; the
    // caller passes dst at the half's first row).  float4 when dst is 16-B
    // aligned (a world group starting off a 4-agent boundary is not).
    template <int n, int P> __device__ __forceinline__ void flushSpan(int h, float *dst) const
    {
        const int total = rowsOf(h) * n;
        auto val = [&](int f) {
            const int r = f / n;
            return buf[r * P + (f - r * n)];
        };
        if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
            const int q4 = total >> 2;
            // rolled, one division per float4 (the four floats walk the
            // staged row and wrap to the next): unrolled, the compiler hoisted
            // per-element LDS offsets out of the loop and held ~40 VGPRs
#pragma unroll 1
            for (int j = lane; j < q4; j += m) {
                int r = (4 * j) / n, c = 4 * j - r * n;
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    v[q] = buf[r * P + c];
                    if (++c == n) {
                        c = 0;
                        r++;
                    }
                }
                reinterpret_cast<float4 *>(dst)[j] = make_float4(v[0], v[1], v[2], v[3]);
            }
            if (lane < (total & 3)) dst[4 * q4 + lane] = val(4 * q4 + lane);
        } else {
#pragma unroll 1
            for (int f = lane; f < total; f += m) dst[f] = val(f);
        }
    }
    // 32-float rows: row r of half h to arr[((gw0 + 32h + r) * slots + k) * 32]
    // as 8 float4 pieces (each store instruction writes 8 whole rows).
    template <int P> __device__ __forceinline__ void flushRows32(int h, float *arr, int slots, int k, int64_t gw0) const
    {
        static_assert(P % 4 == 0, "float4 rows");
        const int nc = rowsOf(h) * (kOtherObs / 4);
        float *base = arr + ((gw0 + 32 * h) * slots + k) * kOtherObs;
        // <= 32 rows x 8 pieces over m >= rows lanes: at most 8 rounds (4 in a full wave)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int c = lane + j * m;
            if (c < nc) {
                const int r = c >> 3, col = c & 7;
                const uint32_t o = (uint32_t)(r * slots * kOtherObs + col * 4); // < 32 rows x 6 slots x 32
                *reinterpret_cast<float4 *>(base + o) = reinterpret_cast<const float4 *>(buf + r * P)[col];
            }
        }
    }
    // Rows of n floats at per-row offsets (offs, staged with stageOff) into
    // dst; wbits / zbits: wave ballots of "row exists" / "row is zeros".
    template <int n, int P> __device__ __forceinline__ void flushOff(int h, float *dst, uint64_t wbits, uint64_t zbits) const
    {
        const uint32_t wb = (uint32_t)(wbits >> (32 * h)), zb = (uint32_t)(zbits >> (32 * h));
        const int total = rowsOf(h) * n;
#pragma unroll 1
        for (int c = lane; c < total; c += m) {
            const int r = c / n, col = c - r * n;
            if ((wb >> r) & 1u) dst[offs[r] + col] = ((zb >> r) & 1u) ? 0.f : buf[r * P + col];
        }
    }
    // The same for rows of n4 float4 (16-B aligned rows, P a multiple of 4).
    template <int n4, int P> __device__ __forceinline__ void flushOff4(int h, float *dst, uint64_t wbits, uint64_t zbits) const
    {
        static_assert(P % 4 == 0, "float4 rows");
        const uint32_t wb = (uint32_t)(wbits >> (32 * h)), zb = (uint32_t)(zbits >> (32 * h));
        const int total = rowsOf(h) * n4;
        for (int c = lane; c < total; c += m) {
            const int r = c / n4, col = c - r * n4;
            if ((wb >> r) & 1u)
                reinterpret_cast<float4 *>(dst + offs[r])[col] =
                    ((zb >> r) & 1u) ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4 *>(buf + r * P)[col];
        }
    }
    // A contiguous span export (lane r's n floats at dst + r * n).
    template <int n> __device__ __forceinline__ void putSpan(float *dst, const float *vals) const
    {
        constexpr int P = n | 1; // odd stride: conflict-free staging
        static_assert(P <= kObsSpanPad, "span larger than the row stage");
        for (int h = 0; h < halves(); h++) {
            stage<P>(h, vals, n);
            waveSync();
            flushSpan<n, P>(h, dst + (int64_t)32 * h * n);
            waveSync();
        }
    }
};

// kWire: the learner's rebuild of a shadow's rows from a wire message
// (wire.hip launchWireUnpack): S is a view whose input columns point into
// the message (the same SoA columns the sender's engine holds), the packed
// pose / weapon / flags word is split here, the full-team rows (not
// trainInterface outputs) are skipped, and a world whose episode counter
// moved since the previous message has every last-known row written -- the
// reset's clear on the sender (resetAgentD / resetPersistentEntitiesD),
// then this step's updates -- exactly the rows the sender's k_obs leaves.
// (One templated kernel, k_obs<false> on the step path and k_obs<true> =
// "k_obs_wire" on the learner: the same body as a __device__ function under
// two kernels compiled ~45% more instructions and ran 6% slower.)
template <bool kWire>
__global__ void __launch_bounds__(kObsBlock) __attribute__((amdgpu_waves_per_eu(3)))
k_obs(DevState S, SceneDev sc, WireObs wo)
{
    __shared__ float ost[kObsCols][kObsStageMax];
    __shared__ __attribute__((aligned(16))) float rowBuf[kObsBlock / 64][32 * kObsSpanPad];
    __shared__ int64_t offBuf[kObsBlock / 64][32];
    // a learner shadow out of wire sync keeps its rows (wire.hip wireOk);
    // the same word for every thread of the grid
    if (S.obsGate && (*S.obsGate & MPENV_WIRE_ERR_DESYNC)) return;
    const int T = S.T, N = S.N;
    const int64_t b0 = (int64_t)xcdBlockId() * kObsBlock; // < A (grid = ceil(A / kObsBlock))
    const int64_t g = b0 + threadIdx.x;
    const bool live = g < S.A;

    // ---- loads: the block's worlds' agent columns, then this lane's own
    // rotation and world fields (no store is issued before all of them)
    const int64_t a_end = b0 + kObsBlock < S.A ? b0 + kObsBlock : S.A;
    const int64_t s0 = (b0 / N) * N;
    const int ns = (int)(((a_end - 1) / N + 1) * N - s0);
    for (int k = threadIdx.x; k < ns; k += kObsBlock) {
        const int64_t j = s0 + k;
        ost[kOsPX][k] = S.px[j];
        ost[kOsPY][k] = S.py[j];
        ost[kOsPZ][k] = S.pz[j];
        ost[kOsVX][k] = S.vx[j];
        ost[kOsVY][k] = S.vy[j];
        ost[kOsVZ][k] = S.vz[j];
        ost[kOsYaw][k] = S.ayaw[j];
        ost[kOsPitch][k] = S.apitch[j];
        ost[kOsDYV][k] = S.dyv[j];
        ost[kOsDPV][k] = S.dpv[j];
        ost[kOsHP][k] = S.hp[j];
        ost[kOsFired][k] = S.firedT[j];
        ost[kOsAlive][k] = S.alive[j];
        if constexpr (kWire) {
            const uint32_t p = wo.packed[j]; // curPose | tgtPose << 8 | weapon << 16 | flags << 24
            ost[kOsCurPose][k] = __int_as_float((int32_t)(p & 0xffu));
            ost[kOsTgtPose][k] = __int_as_float((int32_t)((p >> 8) & 0xffu));
            ost[kOsWeapon][k] = __int_as_float((int32_t)((p >> 16) & 0xffu));
            ost[kOsVis][k] = __int_as_float((int32_t)S.visMask[j]);
            ost[kOsTrans][k] = __int_as_float(S.transRem[j]);
            ost[kOsFlags][k] = __int_as_float((int32_t)(p >> 24));
        } else {
            ost[kOsCurPose][k] = __int_as_float(S.curPose[j]);
            ost[kOsTgtPose][k] = __int_as_float(S.tgtPose[j]);
            ost[kOsWeapon][k] = __int_as_float(S.weapon[j]);
            ost[kOsVis][k] = __int_as_float((int32_t)S.visMask[j]);
            ost[kOsTrans][k] = __int_as_float(S.transRem[j]);
            ost[kOsFlags][k] = __int_as_float(S.flags[j]);
        }
        ost[kOsShot][k] = __int_as_float(S.wasShot[j]);
        ost[kOsHeal][k] = __int_as_float(S.autohealSteps[j]);
        ost[kOsMag0][k] = __int_as_float(S.magazine[2 * j]);
        ost[kOsMag1][k] = __int_as_float(S.magazine[2 * j + 1]);
    }
    const int64_t gs = live ? g : S.A - 1; // tail lanes load a valid agent's fields, then leave
    const int w = (int)(gs / N);
    const int i = (int)(gs - (int64_t)w * N);
    const int team = i / T, off = i - team * T;
    const Quat rot = ldRot(S, gs);
    const int cur_step = S.curStep[w];
    const int fm = team == 0 ? S.filtMatched0[w] : S.filtMatched1[w];
    const int cz = S.curZone[w];
    const int ctrl = S.controlling[w];
    const int contested = S.contested[w], captured = S.captured[w];
    const int until_point = S.stepsUntilPoint[w], zone_steps = S.zoneSteps[w];
    const AABB za = sc.tab->zoneAABB[cz];
    // the pure outputs' destinations: the engine's exports, or during a
    // gpuStreamStep the caller's buffers (OutTab; uniform loads, issued with
    // the other loads before the barrier)
    float *oMasks = S.masks, *oFilters = S.filters, *oSelf = S.selfObs, *oSelfPos = S.selfPos;
    float *oTm = S.tmObs, *oTmPos = S.tmPos, *oOpp = S.oppObs, *oOppPos = S.oppPos;
    if (!kWire && S.outTab && S.outTab->on) {
        const OutTab *t = S.outTab;
        const int64_t b = S.outBase;
        oMasks = t->masks + b * 6;
        oFilters = t->filters + b;
        oSelf = t->selfObs + b * kSelfObs;
        oSelfPos = t->selfPos + b * 3;
        oTm = t->tmObs + b * 5 * kOtherObs;
        oTmPos = t->tmPos + b * 15;
        oOpp = t->oppObs + b * 6 * kOtherObs;
        oOppPos = t->oppPos + b * 18;
    }
    bool wreset = false; // kWire: the world's episode counter moved since the previous message
    if constexpr (kWire) wreset = !wo.keyframe && wo.epPrev[w] != S.episodeCounter[w];
    __syncthreads();
    if (!live) return; // the flushes count the live lanes

    const ObsStage st { ost };
    const int lane = threadIdx.x & 63;
    const int64_t gw0 = g - lane; // first agent of the wave
    HalfStage hs;
    hs.buf = rowBuf[threadIdx.x >> 6];
    hs.offs = offBuf[threadIdx.x >> 6];
    hs.lane = lane;
    hs.m = (int)(S.A - gw0 < 64 ? S.A - gw0 : 64);
    const int64_t g0 = (int64_t)w * N;
    const int me = (int)(g - s0), l0 = (int)(g0 - s0); // stage indices: this agent, its world's first
    const bool self_alive = st.alive(me);

    // ---- masks
    float mask[kMaxTeamSize];
    for (int k = 0; k < kMaxTeamSize; k++) {
        mask[k] = 0.f;
        if (!self_alive || k >= T) continue;
        const int jo = l0 + (team ^ 1) * T + k;
        if (!st.alive(jo)) continue;
        bool can_see = (st.i(kOsVis, me) >> k) & 1;
        for (int t = 0; t < T - 1 && !can_see; t++) {
            const int jt = l0 + team * T + (t < off ? t : t + 1);
            if ((st.i(kOsVis, jt) >> k) & 1) can_see = true;
        }
        if (can_see) mask[k] = 1.f;
        if (st.f(kOsFired, jo) >= 0) mask[k] = 1.f;
    }
    hs.putSpan<6>(oMasks + gw0 * 6, mask);
    // teamKnowsLocation (mask[k] == 1) as bits for the opponent loop.
    // Reading the float array there instead gave wrong last-known updates in
    // round 2 -- a register miscompile of the float form ("k_obs
    // mask read"); the bits form is taken right here.
    uint32_t knowsBits = 0;
    for (int k = 0; k < kMaxTeamSize; k++) knowsBits |= (mask[k] == 1.f ? 1u : 0u) << k;

    oFilters[g] = (cur_step - fm < 5) ? 1.f : 0.f;

    // ---- fullTeamObservationsSystem, per (world, team): the global
    // observation and the zeroed slots past team_size (slot-0 agents)
    const int64_t mine = (int64_t)w * 2 + team, theirs = (int64_t)w * 2 + (team ^ 1);
    if (!kWire && off == 0) {
        for (int s = T; s < kMaxTeamSize; s++) {
            for (int k = 0; k < MPENV_FT_PLAYER_DIM; k++) S.ftPlayers[(mine * 6 + s) * MPENV_FT_PLAYER_DIM + k] = 0.f;
            for (int k = 0; k < MPENV_FT_ENEMY_DIM; k++) S.ftEnemies[(mine * 6 + s) * MPENV_FT_ENEMY_DIM + k] = 0.f;
            for (int k = 0; k < MPENV_FT_COMMON_DIM; k++) S.ftLastKnown[(mine * 6 + s) * MPENV_FT_COMMON_DIM + k] = 0.f;
        }
        float gob[MPENV_FT_GLOBAL_DIM];
        gob[0] = team == 0 ? 0.f : 1.f;
        gob[1] = team == 0 ? 1.f : 0.f;
        gob[2] = float(c::kEpisodeLen - cur_step) / c::kEpisodeLen;
        const Vec3 nc = normalizedPosUnclampedD(sc, (za.pMax + za.pMin) / 2.f);
        gob[3] = nc.x; gob[4] = nc.y; gob[5] = nc.z;
        gob[6] = ctrl == team ? 1.f : 0.f;
        gob[7] = (ctrl != -1 && ctrl != team) ? 1.f : 0.f;
        gob[8] = contested ? 1.f : 0.f;
        gob[9] = captured ? 1.f : 0.f;
        gob[10] = float(until_point) / float(c::kZonePointInterval);
        gob[11] = float(zone_steps) / float(c::kNumStepsPerZone);
        for (int k = 0; k < 4; k++) gob[12 + k] = cz == k ? 1.f : 0.f;
        static_assert(MPENV_FT_GLOBAL_DIM == 16, "ft global row: 4 float4");
        float4 *gdst = reinterpret_cast<float4 *>(&S.ftGlobal[mine * MPENV_FT_GLOBAL_DIM]);
        for (int q = 0; q < 4; q++) gdst[q] = make_float4(gob[4 * q], gob[4 * q + 1], gob[4 * q + 2], gob[4 * q + 3]);
    }

    // ---- self observation
    SelfFrame sf;
    sf.pos = st.pos(me);
    sf.invRot = qinv(rot);
    sf.yaw = st.f(kOsYaw, me);
    sf.pitch = st.f(kOsPitch, me);
    {
        float ob[kSelfObs];
        float pos3[3];
        for (int k = 0; k < kSelfObs; k++) ob[k] = 0.f;
        pos3[0] = pos3[1] = pos3[2] = -1000.f;
        if (fillCommonS(st, sc, sf, me, ob, pos3)) {
            fillCombatS(st, me, &ob[23]);
            float *zo = &ob[27];
            Vec3 center = (za.pMax + za.pMin) / 2.f;
            Vec3 nc = normalizedPosD(sc, center);
            zo[0] = nc.x; zo[1] = nc.y; zo[2] = nc.z;
            relAnglesD(sf, center - sf.pos, zo[3], zo[4], zo[5]);
            zo[6] = (ctrl == team) ? 1.f : 0.f;
            zo[7] = (ctrl != -1 && ctrl != team) ? 1.f : 0.f;
            zo[8] = contested ? 1.f : 0.f;
            zo[9] = captured ? 1.f : 0.f;
            zo[10] = float(until_point) / float(c::kZonePointInterval);
            zo[11] = float(zone_steps) / float(c::kNumStepsPerZone);
            zo[12] = cz == 0 ? 1.f : 0.f;
            zo[13] = cz == 1 ? 1.f : 0.f;
            zo[14] = cz == 2 ? 1.f : 0.f;
            zo[15] = cz == 3 ? 1.f : 0.f;
        }
        static_assert(kSelfObs == 43 && (kSelfObs | 1) <= kObsSpanPad, "self obs span");
        hs.putSpan<kSelfObs>(oSelf + gw0 * kSelfObs, ob);
        hs.putSpan<3>(oSelfPos + gw0 * 3, pos3);
    }
    const bool alive_ok = self_alive; // fillCommonOb's alive test of the agent itself

    // Slot positions (teammate, opponent, last-known rows) are recomputed
    // after each slot loop in fully unrolled form: written from inside the
    // rolled loops, the arrays were indexed dynamically and went to scratch,
    // whose loads would wait behind the row stores.
    auto slotPos = [&](bool exists, int j, float *p3) {
        if (exists && st.alive(j)) {
            const Vec3 np = normalizedPosD(sc, st.pos(j));
            p3[0] = np.x; p3[1] = np.y; p3[2] = np.z;
        } else {
            p3[0] = p3[1] = p3[2] = -1000.f;
        }
    };
    auto mateIdx = [&](int k) { return l0 + team * T + (k < off ? k : k + 1); };
    auto oppIdx = [&](int k) { return l0 + (team ^ 1) * T + k; };

    // ---- teammates
    {
        for (int k = 0; k < kMaxTeamSize - 1; k++) {
            float row[kOtherObs];
            float unused[3];
            for (int q = 0; q < kOtherObs; q++) row[q] = 0.f;
            if (alive_ok && k < T - 1) {
                const int jt = mateIdx(k);
                if (fillCommonS(st, sc, sf, jt, row, unused)) {
                    fillOtherS(st, sf, jt, row);
                    fillCombatS(st, jt, &row[28]);
                }
            }
            for (int h = 0; h < hs.halves(); h++) {
                hs.stage<kObsRowPad>(h, row, kOtherObs);
                waveSync();
                hs.flushRows32<kObsRowPad>(h, oTm, 5, k, gw0);
                waveSync();
            }
        }
        float tpos[15];
#pragma unroll
        for (int k = 0; k < kMaxTeamSize - 1; k++) slotPos(alive_ok && k < T - 1, mateIdx(k), &tpos[3 * k]);
        hs.putSpan<15>(oTmPos + gw0 * 15, tpos);
    }

    // ---- opponents (+ last known)
    {
        uint32_t lkWrite = 0, lkKeep = 0; // per slot: last-known row written / kept (else cleared)
        for (int k = 0; k < kMaxTeamSize; k++) {
            float row[kOtherObs];
            float unused[3];
            for (int q = 0; q < kOtherObs; q++) row[q] = 0.f;
            // last-known slot: cleared (opponent dead / just killed), then
            // overwritten with the observation when the team knows the location
            bool lk_write = false, lk_keep = false;
            if (alive_ok && k < T) {
                const int jo = oppIdx(k);
                if (!fillCommonS(st, sc, sf, jo, row, unused)) {
                    lk_write = true;
                } else {
                    fillOtherS(st, sf, jo, row);
                    if (st.i(kOsFlags, jo) & kFlagWasKilled) lk_write = true;
                    row[28] = (float)st.i(kOsShot, jo);
                    row[29] = st.f(kOsFired, jo) >= 0.f ? 1.f : 0.f;
                    row[30] = ((st.i(kOsVis, me) >> k) & 1) ? 1.f : 0.f;
                    // teamKnowsLocation (sim.cpp:2995-3003)
                    const bool knows = (knowsBits >> k) & 1u;
                    row[31] = knows ? 1.f : 0.f;
                    lk_keep = knows;
                    lk_write = lk_write || knows;
                }
            }
            lk_write = lk_write || wreset;
            lkWrite |= (lk_write ? 1u : 0u) << k;
            lkKeep |= (lk_keep ? 1u : 0u) << k;
            if (S.stats) statAdd(S.stats + kStatLkRows, lk_write ? 1u : 0u);
            const uint64_t wb = __ballot(lk_write), zb = __ballot(!lk_keep);
            for (int h = 0; h < hs.halves(); h++) {
                hs.stage<kObsRowPad>(h, row, kOtherObs);
                hs.stageOff(h, (g * 6 + k) * kOtherObs);
                waveSync();
                hs.flushRows32<kObsRowPad>(h, oOpp, 6, k, gw0);
                // the staged row is also the last-known copy
                hs.flushOff4<kOtherObs / 4, kObsRowPad>(h, S.lkObs, wb, zb);
                waveSync();
            }
        }
        float opos[18];
#pragma unroll
        for (int k = 0; k < kMaxTeamSize; k++) slotPos(alive_ok && k < T, oppIdx(k), &opos[3 * k]);
        hs.putSpan<18>(oOppPos + gw0 * 18, opos);
        // last-known positions: the written slots of each row (kept: the
        // observed position, cleared: -1000)
        {
            float lpos[18];
#pragma unroll
            for (int q = 0; q < 18; q++) lpos[q] = ((lkKeep >> (q / 3)) & 1u) ? opos[q] : -1000.f;
            constexpr int P = 19;
            for (int h = 0; h < hs.halves(); h++) {
                hs.stage<P>(h, lpos, 18);
                hs.stageOff(h, (int64_t)lkWrite); // the row's slot mask (rows at g * 18)
                waveSync();
                const int total = hs.rowsOf(h) * 18;
                float *dst = S.lkPos + (gw0 + 32 * h) * 18;
#pragma unroll 1
                for (int c = lane; c < total; c += hs.m) {
                    const int r = c / 18, col = c - r * 18;
                    if ((hs.offs[r] >> (col / 3)) & 1) dst[c] = hs.buf[r * P + col];
                }
                waveSync();
            }
        }
    }

    // ---- fullTeamObservationsSystem, the part owned by agent g (team, slot
    // off): its player slot in its own team's interface, its enemy and
    // last-known slots in the other team's interface (the common block is the
    // same in all three, the one-hot id is the slot).  Positions are
    // normalised without the clamp pvpObservations applies.  The lidar copy is
    // fused into k_lidar.
    if constexpr (!kWire) {
        const bool alive = self_alive;
        // enemy-only fields first: they decide whether the last-known slot
        // receives the common block
        const float fired = alive && st.f(kOsFired, me) >= 0.f ? 1.f : 0.f;
        bool knows = fired != 0.f;
        uint32_t los = 0;
        if (alive) {
            const int jm0 = l0 + (team ^ 1) * T;
            for (int mm = 0; mm < T; mm++) los |= ((st.i(kOsVis, jm0 + mm) >> off) & 1u) << mm;
            knows = knows || los != 0;
        }
        float cm[MPENV_FT_ENEMY_DIM]; // the common block, then the enemy tail
        cm[0] = 1.f;
        for (int k = 0; k < kMaxTeamSize; k++) cm[1 + k] = k == off ? 1.f : 0.f;
        for (int k = 7; k < MPENV_FT_COMMON_DIM; k++) cm[k] = 0.f;
        float ext[4] = { 0.f, 0.f, 0.f, 0.f };
        if (alive) {
            cm[7] = 1.f;
            const Vec3 np = normalizedPosUnclampedD(sc, st.pos(me));
            cm[8] = np.x; cm[9] = np.y; cm[10] = np.z;
            cm[11] = 0.5f * ((st.f(kOsYaw, me) / kPi) + 1.f);
            cm[12] = 0.5f * (st.f(kOsPitch, me) / (0.25f * kPi) + 1.f);
            cm[13] = st.f(kOsVX, me); cm[14] = st.f(kOsVY, me); cm[15] = st.f(kOsVZ, me);
            const int cp = st.i(kOsCurPose, me), tp = st.i(kOsTgtPose, me);
            cm[16] = cp == kStand ? 1.f : 0.f;
            cm[17] = cp == kCrouch ? 1.f : 0.f;
            cm[18] = cp == kProne ? 1.f : 0.f;
            cm[19] = tp == kStand ? 1.f : 0.f;
            cm[20] = tp == kCrouch ? 1.f : 0.f;
            cm[21] = tp == kProne ? 1.f : 0.f;
            cm[22] = (float)st.i(kOsTrans, me) / (float)c::kPoseTransitionSpeed;
            cm[23] = (st.i(kOsFlags, me) & kFlagInZone) ? 1.f : 0.f;
            ext[0] = st.f(kOsHP, me) / 100.f;
            ext[1] = (float)st.i(kOsMag0, me) / 30;
            ext[2] = (float)st.i(kOsMag1, me);
            ext[3] = float(st.i(kOsHeal, me)) / float(c::kOutOfCombatSteps);
        }
        cm[MPENV_FT_COMMON_DIM + 0] = alive ? (float)st.i(kOsShot, me) : 0.f;
        cm[MPENV_FT_COMMON_DIM + 1] = fired;
        for (int mm = 0; mm < kMaxTeamSize; mm++) cm[MPENV_FT_COMMON_DIM + 2 + mm] = (los >> mm) & 1u ? 1.f : 0.f;
        cm[MPENV_FT_COMMON_DIM + 8] = knows ? 1.f : 0.f;
        static_assert(MPENV_FT_ENEMY_DIM == MPENV_FT_COMMON_DIM + 9, "ft enemy tail");
        // one staged row serves all three slots: the common block + enemy
        // tail; the player tail is staged over the enemy tail after the
        // enemy row has left
        constexpr int P = kObsRowPad;
        static_assert(MPENV_FT_ENEMY_DIM <= P && MPENV_FT_PLAYER_DIM <= P, "ft rows");
        static_assert(MPENV_FT_COMMON_DIM % 4 == 0 && MPENV_FT_PLAYER_DIM % 4 == 0, "16-B ft rows");
        const uint64_t all = __ballot(true), zlk = __ballot(!knows);
        for (int h = 0; h < hs.halves(); h++) {
            hs.stage<P>(h, cm, MPENV_FT_ENEMY_DIM);
            hs.stageOff(h, (theirs * 6 + off) * MPENV_FT_ENEMY_DIM);
            waveSync();
            hs.flushOff<MPENV_FT_ENEMY_DIM, P>(h, S.ftEnemies, all, 0ull);
            waveSync();
            hs.stage<P>(h, ext, 4, MPENV_FT_COMMON_DIM);
            hs.stageOff(h, (theirs * 6 + off) * MPENV_FT_COMMON_DIM);
            waveSync();
            hs.flushOff4<MPENV_FT_COMMON_DIM / 4, P>(h, S.ftLastKnown, all, zlk);
            waveSync();
            hs.stageOff(h, (mine * 6 + off) * MPENV_FT_PLAYER_DIM);
            waveSync();
            hs.flushOff4<MPENV_FT_PLAYER_DIM / 4, P>(h, S.ftPlayers, all, 0ull);
            waveSync();
        }
    }
}

// ============================================================ host side
int launchObservations(const DevState &s, const SceneDev &sc, void *stream)
{
    const int blocks = (int)((s.A + kObsBlock - 1) / kObsBlock);
    hipLaunchKernelGGL(k_obs<false>, dim3(blocks), dim3(kObsBlock), 0, (hipStream_t)stream, s, sc, WireObs {});
    return check(hipGetLastError());
}

int launchObservationsWire(const DevState &view, const SceneDev &sc, const WireObs &wo, void *stream)
{
    const int blocks = (int)((view.A + kObsBlock - 1) / kObsBlock);
    hipLaunchKernelGGL(k_obs<true>, dim3(blocks), dim3(kObsBlock), 0, (hipStream_t)stream, view, sc, wo);
    return check(hipGetLastError());
}

} // namespace mpenv
