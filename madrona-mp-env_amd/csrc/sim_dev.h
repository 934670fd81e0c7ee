// sim_dev.h — what the kernel files of the step share (kernels.hip, move.hip,
// hooks.hip): the reference's constants, the SoA accessors, the block size
// and block order, and the launchers' error check and launch by residency.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.h"
#include "geom_dev.h"

// (file scope: holds for the rest of every translation unit that includes this)
#pragma clang fp contract(off)

namespace mpenv {

using namespace mp;

// ----------------------------------------------------- consts.hpp:7-72
namespace c {
constexpr int kNumStepsPerZone = 600;
constexpr int kZonePointInterval = 20;
constexpr int kZoneWinPoints = 125;
constexpr int kPoseTransitionSpeed = 10;
constexpr float kAgentRadius = 15.f;
constexpr float kStandHeight = 65.f;
constexpr float kCrouchHeight = 47.f;
constexpr float kProneHeight = 30.f;
constexpr float kMaxRunVelocity = 400.f;
constexpr float kMaxWalkVelocity = 200.f;
constexpr float kMaxCrouchVelocity = 50.f;
constexpr float kMaxProneVelocity = 20.f;
constexpr float kDeaccelerateRate = 1000.f;
constexpr int kRespawnInvincibleSteps = 5;
constexpr int kOutOfCombatSteps = 150;
constexpr float kAutohealPerStep = 5.f;
constexpr int kEpisodeLen = 3000;
constexpr int kNumMoveAmountBuckets = 3;
constexpr int kNumMoveAngleBuckets = 8;
constexpr float kDeltaT = 0.05f;
constexpr int kDiscreteAimYawBuckets = 13;
constexpr int kDiscreteAimPitchBuckets = 7;
constexpr int kGridMax = 40;
// mgr.cpp:1383-1395 weapon stats
constexpr int kMagSize = 30;
constexpr int kReloadTime = 30;
constexpr float kDmgPerBullet = 10.f;
constexpr float kAccuracyScale = 0.005f;
constexpr int kNumWeaponTypes = 1;
} // namespace c

enum { kStand = 0, kCrouch = 1, kProne = 2 };
constexpr uint32_t kFlagNoRespawn = 1u << 3;
constexpr uint32_t kFlagSpawnInMiddle = 1u << 0;
constexpr uint32_t kFlagRandomizeHP = 1u << 1;
constexpr uint32_t kFlagHardcodedSpawns = 1u << 6;
constexpr uint32_t kFlagEnableCurriculum = 1u << 5;
constexpr uint32_t kFlagNavmeshSpawn = 1u << 2;
constexpr uint32_t kFlagSubZones = 1u << 11;

__device__ __forceinline__ float viewHeightD(int pose)
{
    float top = pose == kStand ? c::kStandHeight : (pose == kCrouch ? c::kCrouchHeight : c::kProneHeight);
    return top - c::kAgentRadius;
}

__device__ __forceinline__ int32_t f2iSatD(float f)
{
    if (!(f == f)) return 0;
    if (f >= 2147483520.f) return INT32_MAX;
    if (f <= -2147483648.f) return INT32_MIN;
    return (int32_t)f;
}

// ------------------------------------------------------ SoA accessors
__device__ __forceinline__ Vec3 ldPos(const DevState &S, int64_t g) { return v3(S.px[g], S.py[g], S.pz[g]); }
__device__ __forceinline__ void stPos(const DevState &S, int64_t g, Vec3 p) { S.px[g] = p.x; S.py[g] = p.y; S.pz[g] = p.z; }
__device__ __forceinline__ Vec3 ldVel(const DevState &S, int64_t g) { return v3(S.vx[g], S.vy[g], S.vz[g]); }
__device__ __forceinline__ void stVel(const DevState &S, int64_t g, Vec3 v) { S.vx[g] = v.x; S.vy[g] = v.y; S.vz[g] = v.z; }
__device__ __forceinline__ Quat ldRot(const DevState &S, int64_t g) { return quat(S.rw[g], S.rx[g], S.ry[g], S.rz[g]); }
__device__ __forceinline__ void stRot(const DevState &S, int64_t g, Quat q) { S.rw[g] = q.w; S.rx[g] = q.x; S.ry[g] = q.y; S.rz[g] = q.z; }
__device__ __forceinline__ Quat ldAimRot(const DevState &S, int64_t g) { return quat(S.aw[g], S.ax[g], S.ay[g], S.az[g]); }
__device__ __forceinline__ void stAimRot(const DevState &S, int64_t g, Quat q) { S.aw[g] = q.w; S.ax[g] = q.x; S.ay[g] = q.y; S.az[g] = q.z; }
__device__ __forceinline__ RNG ldRng(const DevState &S, int64_t g)
{
    RNG r; r.key.a = (uint32_t)S.rngA[g]; r.key.b = (uint32_t)S.rngB[g]; r.ctr = (uint32_t)S.rngCtr[g];
    return r;
}
__device__ __forceinline__ void stRng(const DevState &S, int64_t g, const RNG &r)
{
    S.rngA[g] = (int32_t)r.key.a; S.rngB[g] = (int32_t)r.key.b; S.rngCtr[g] = (int32_t)r.ctr;
}
__device__ __forceinline__ RNG ldWRng(const DevState &S, int w)
{
    RNG r; r.key.a = (uint32_t)S.wRngA[w]; r.key.b = (uint32_t)S.wRngB[w]; r.ctr = (uint32_t)S.wRngCtr[w];
    return r;
}
__device__ __forceinline__ void stWRng(const DevState &S, int w, const RNG &r)
{
    S.wRngA[w] = (int32_t)r.key.a; S.wRngB[w] = (int32_t)r.key.b; S.wRngCtr[w] = (int32_t)r.ctr;
}
__device__ __forceinline__ void setFlag(const DevState &S, int64_t g, int32_t bit, bool v)
{
    int32_t f = S.flags[g];
    S.flags[g] = v ? (f | bit) : (f & ~bit);
}

struct AimD {
    float yaw, pitch;
    Quat rot;
};

// utils.cpp:140-167 computeAim
__device__ __forceinline__ AimD computeAimD(float yaw, float pitch)
{
    if (yaw < -kPi) yaw += 2.f * kPi;
    else if (yaw > kPi) yaw -= 2.f * kPi;
    if (pitch < -0.25f * kPi) pitch = -0.25f * kPi;
    if (pitch > 0.25f * kPi) pitch = 0.25f * kPi;
    Quat r = angleAxis(yaw, kUp) * angleAxis(pitch, kRight);
    r = qnormalize(r);
    AimD a;
    a.yaw = yaw; a.pitch = pitch; a.rot = r;
    return a;
}

__device__ __forceinline__ void stAim(const DevState &S, int64_t g, const AimD &a)
{
    S.ayaw[g] = a.yaw; S.apitch[g] = a.pitch; stAimRot(S, g, a.rot);
}

constexpr int kBlock = 256;

// XCD-aware block order (cdna_hip_programming.md T1): the dispatcher deals
// consecutive blocks round-robin to the 8 XCDs, each with its own L2; the
// step kernels index worlds / agents by block, so neighbouring blocks share
// cache lines of the per-world and per-agent columns.  Renumbered, each XCD
// runs one contiguous range of blocks (bijective for any grid size).
__device__ __forceinline__ uint32_t xcdBlockId()
{
    const uint32_t nwg = gridDim.x, orig = blockIdx.x;
    const uint32_t xcd = orig % 8u, q = nwg / 8u, r = nwg % 8u;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + orig / 8u;
}

// Breadcrumb rows and explore-bitset addressing (k_sim writes them, k_debug reads them).
__device__ __forceinline__ float4 *crumbPtr(const DevState &S, int w) { return &S.crumbs[(int64_t)w * kMaxCrumbs * 2]; }
__device__ __forceinline__ int exploreBitD(int cx, int cy) { return (cy & 7) * 8 + (cx & 7); }
__device__ __forceinline__ int exploreTileD(int cx, int cy) { return (cy >> 3) * kExploreTilesX + (cx >> 3); }

static int check(hipError_t e) { return e == hipSuccess ? 0 : -1; }

// Launches a BVH kernel by the images' residency: `lds`, which stages them into `ldsBytes` (its
// *LdsBytes(sc, img.residency)) of dynamic LDS, or `glb`, its `_g` twin with the images as one more parameter.
template <class... P>
static int launchByResidency(const SceneImages &img, void (*lds)(P...), void (*glb)(P..., SceneImages), dim3 grid,
                             dim3 block, size_t ldsBytes, void *stream, const P &...args)
{
    if (img.residency == kResidencyGlobal)
        hipLaunchKernelGGL(glb, grid, block, ldsBytes, (hipStream_t)stream, args..., img);
    else
        hipLaunchKernelGGL(lds, grid, block, ldsBytes, (hipStream_t)stream, args...);
    return check(hipGetLastError());
}

} // namespace mpenv
