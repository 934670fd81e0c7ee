// policy_ref.cpp — TEST INFRASTRUCTURE: an independent CPU restatement of
// in-sim policy inference (DESIGN.md §2 definition 15; the reference's
// evalAgentPolicy, src/dnn.cpp:555-891), one agent at a time in the
// reference's order.  Built by tests/policy_testlib.py with
//   g++ -O2 -ffp-contract=off -fno-fast-math
// and loaded with ctypes.  Shares only csrc/mpenv_core.h (sinf_, cosf_,
// logf_, sqrt_, the RNG) with the engine.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mpenv_core.h"

using std::size_t;

namespace {

constexpr int kEmbed = 64, kHidden = 512, kSelfObs = 43, kCoefs = 9, kOther = 32;
constexpr int kSelfIn = kSelfObs + kCoefs + 48;
constexpr int kBuckets[6] = { 3, 8, 3, 3, 13, 7 }; // moveAmount, moveAngle, fire, stand, yaw, pitch
constexpr int kLogits = 37;

const float kNegInf = mp::u2f(0xff800000u);

// [K][N] -> [N][K], so that a chain walks memory in order (dnn.cpp:1125-1133)
std::vector<float> transposed(const float *w, int K, int N)
{
    std::vector<float> t((size_t)K * N);
    for (int k = 0; k < K; k++)
        for (int n = 0; n < N; n++) t[(size_t)n * K + k] = w[(size_t)k * N + n];
    return t;
}

// y = fmaf(a[K-1], x[K-1], ... fmaf(a[0], x[0], +0.f)) (dnn.cpp:416-421, with
// the product and the sum fused: definition 15)
float chain(const float *a, const float *x, int K)
{
    float y = 0.f;
    for (int k = 0; k < K; k++) y = __builtin_fmaf(a[k], x[k], y);
    return y;
}

struct Layer {
    std::vector<float> wt; // [N][K]
    const float *scale, *bias;
    int K, N;
};

// dense, Welford LayerNorm over the outputs in index order, leaky ReLU (dnn.cpp:428-524)
void layerNormDense(const Layer &l, const float *x, float slope, float *out)
{
    float mean = 0.f, m2 = 0.f;
    for (int i = 0; i < l.N; i++) {
        const float y = chain(&l.wt[(size_t)i * l.K], x, l.K);
        out[i] = y;
        const float delta = y - mean;
        mean = __builtin_fmaf(delta, 1.f / (float)(i + 1), mean);
        const float delta2 = y - mean;
        m2 = __builtin_fmaf(delta, delta2, m2);
    }
    const float sigma = mp::sqrt_(m2 / (float)l.N + 1e-6f);
    for (int i = 0; i < l.N; i++) {
        const float r = __builtin_fmaf(l.scale[i] / sigma, out[i] - mean, l.bias[i]);
        out[i] = r >= 0.f ? r : slope * r;
    }
}

void normalise(const float *x, int n, const float *mean, const float *inv, int period, float *out)
{
    for (int i = 0; i < n; i++) out[i] = inv[i % period] * (x[i] - mean[i % period]);
}

void posEmbed(const float *p, float *out)
{
    for (int i = 0; i < 8; i++)
        for (int c = 0; c < 3; c++) {
            const float scaled = p[c] * (float)(1 << i) * mp::kPi;
            out[(2 * i) * 3 + c] = mp::sinf_(scaled);
            out[(2 * i + 1) * 3 + c] = mp::cosf_(scaled);
        }
}

float gumbel(float u) { return -mp::logf_(-mp::logf_(u)); }

int32_t sampleHead(const float *lg, int nb, mp::RandKey k)
{
    int32_t best = 0;
    float mx = kNegInf;
    for (int i = 0; i < nb; i++) {
        const float score = lg[i] + gumbel(mp::keyUniform(mp::splitI(k, (uint32_t)i)));
        if (score > mx) {
            mx = score;
            best = i;
        }
    }
    return best;
}

} // namespace

extern "C" {

// order of the 7 normalisation sets: self, coefs, fwd, rear, teammates, opponents, last-known;
// of the 6 embed modules: self, fwd, rear, teammates, opponents, last-known
struct PolicyRefWeights {
    const float *normMean[7], *normInv[7];
    const float *embedW[6], *embedScale[6], *embedBias[6]; // kernels [in][64]
    const float *trunkW[3], *trunkScale[3], *trunkBias[3]; // [384 | 512][512]
    const float *headW[2], *headBias[2];                   // [512][17], [512][20]
};

void policy_ref_dense(const float *x, int M, int K, const float *w, int N, float *y)
{
    const std::vector<float> wt = transposed(w, K, N);
    for (int m = 0; m < M; m++)
        for (int n = 0; n < N; n++) y[(size_t)m * N + n] = chain(&wt[(size_t)n * K], x + (size_t)m * K, K);
}

void policy_ref_pos_embed(const float *pos3, float *out48) { posEmbed(pos3, out48); }

float policy_ref_gumbel(float u) { return gumbel(u); }

int32_t policy_ref_sample_head(const float *logits, int nb, uint32_t key_a, uint32_t key_b)
{
    mp::RandKey k;
    k.a = key_a;
    k.b = key_b;
    return sampleHead(logits, nb, k);
}

// logits [n][37]; trunk_in [n][384] optional
void policy_ref_forward(int n, const float *selfObs, const float *coefs, const float *selfPos, const float *fwd,
                        const float *rear, const float *tm, const float *opp, const float *masks, const float *lk,
                        const PolicyRefWeights *W, float *logits, float *trunk_in)
{
    const int modIn[6] = { kSelfIn, 256, 64, kOther, kOther, kOther };
    Layer emb[6], trunk[3];
    for (int m = 0; m < 6; m++)
        emb[m] = Layer { transposed(W->embedW[m], modIn[m], kEmbed), W->embedScale[m], W->embedBias[m], modIn[m], kEmbed };
    for (int i = 0; i < 3; i++) {
        const int K = i == 0 ? 6 * kEmbed : kHidden;
        trunk[i] = Layer { transposed(W->trunkW[i], K, kHidden), W->trunkScale[i], W->trunkBias[i], K, kHidden };
    }
    const int headN[2] = { 17, 20 };
    std::vector<float> headT[2] = { transposed(W->headW[0], kHidden, 17), transposed(W->headW[1], kHidden, 20) };

    for (int a = 0; a < n; a++) {
        float in[6 * kEmbed], x[256], e[kEmbed];
        // self (dnn.cpp:593-624)
        normalise(selfObs + (size_t)a * kSelfObs, kSelfObs, W->normMean[0], W->normInv[0], kSelfObs, x);
        normalise(coefs + (size_t)a * kCoefs, kCoefs, W->normMean[1], W->normInv[1], kCoefs, x + kSelfObs);
        posEmbed(selfPos + (size_t)a * 3, x + kSelfObs + kCoefs);
        layerNormDense(emb[0], x, 1e-2f, in);
        // lidar (dnn.cpp:626-648)
        normalise(fwd + (size_t)a * 256, 256, W->normMean[2], W->normInv[2], 4, x);
        layerNormDense(emb[1], x, 1e-2f, in + kEmbed);
        normalise(rear + (size_t)a * 64, 64, W->normMean[3], W->normInv[3], 4, x);
        layerNormDense(emb[2], x, 1e-2f, in + 2 * kEmbed);
        // teammates, opponents (masked), last-known: max over every slot from -inf (dnn.cpp:650-726)
        const float *slots[3] = { tm + (size_t)a * 5 * kOther, opp + (size_t)a * 6 * kOther, lk + (size_t)a * 6 * kOther };
        const int numSlots[3] = { 5, 6, 6 };
        for (int g = 0; g < 3; g++) {
            float *cur = in + (3 + g) * kEmbed;
            for (int i = 0; i < kEmbed; i++) cur[i] = kNegInf;
            for (int s = 0; s < numSlots[g]; s++) {
                normalise(slots[g] + s * kOther, kOther, W->normMean[4 + g], W->normInv[4 + g], kOther, x);
                layerNormDense(emb[3 + g], x, 1e-2f, e);
                const float mask = g == 1 ? masks[(size_t)a * 6 + s] : 1.f;
                for (int i = 0; i < kEmbed; i++) cur[i] = mp::fmaxD(cur[i], g == 1 ? mask * e[i] : e[i]);
            }
        }
        if (trunk_in)
            for (int i = 0; i < 6 * kEmbed; i++) trunk_in[(size_t)a * 6 * kEmbed + i] = in[i];
        // trunk and heads (dnn.cpp:740-840)
        float h0[kHidden], h1[kHidden];
        layerNormDense(trunk[0], in, 0.f, h0);
        layerNormDense(trunk[1], h0, 0.f, h1);
        layerNormDense(trunk[2], h1, 0.f, h0);
        float *lg = logits + (size_t)a * kLogits;
        for (int h = 0; h < 2; h++) {
            for (int i = 0; i < headN[h]; i++) lg[i] = chain(&headT[h][(size_t)i * kHidden], h0, kHidden) + W->headBias[h][i];
            lg += headN[h];
        }
    }
}

// actions [n][6] from logits [n][37] and each agent's RNG; ctr_out (optional) = ctr + 6
void policy_ref_sample(int n, const float *logits, const int32_t *rngA, const int32_t *rngB, const int32_t *rngCtr,
                       int32_t *actions, int32_t *ctr_out)
{
    for (int a = 0; a < n; a++) {
        mp::RNG rng;
        rng.key.a = (uint32_t)rngA[a];
        rng.key.b = (uint32_t)rngB[a];
        rng.ctr = (uint32_t)rngCtr[a];
        const float *lg = logits + (size_t)a * kLogits;
        for (int h = 0; h < 6; h++) {
            actions[(size_t)a * 6 + h] = sampleHead(lg, kBuckets[h], mp::rngAdvance(rng));
            lg += kBuckets[h];
        }
        if (ctr_out) ctr_out[a] = (int32_t)rng.ctr;
    }
}

// the Gumbel noise policy_ref_sample adds: g [n][37], bucket by bucket in head order
void policy_ref_gumbels(int n, const int32_t *rngA, const int32_t *rngB, const int32_t *rngCtr, float *g)
{
    for (int a = 0; a < n; a++) {
        mp::RNG rng;
        rng.key.a = (uint32_t)rngA[a];
        rng.key.b = (uint32_t)rngB[a];
        rng.ctr = (uint32_t)rngCtr[a];
        float *out = g + (size_t)a * kLogits;
        for (int h = 0; h < 6; h++) {
            const mp::RandKey k = mp::rngAdvance(rng);
            for (int i = 0; i < kBuckets[h]; i++) *out++ = gumbel(mp::keyUniform(mp::splitI(k, (uint32_t)i)));
        }
    }
}

} // extern "C"
