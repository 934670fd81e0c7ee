// policy.cpp — the frozen-checkpoint loader of in-sim policy inference
// (DESIGN.md §2 definition 15).  Reads the reference's converted-checkpoint
// directory (loadWeightFile, dnn.cpp:1066-1090: i32 ndim, i32 shape[ndim], f32
// data; kernels [in][out]) and checks every rank and shape against the fixed
// architecture, where the reference asserts (dnn.cpp:1107,1116-1117,1156,
// 1163-1164,1182-1183,...).  Needs no GPU.
#include <hip/hip_runtime.h> // engine.h's vector types

#include <cstdio>
#include <cstring>

#include "policy.h"

namespace mpenv {

void pol::packB(const float *w, int K, int N, float *out)
{
    const int steps = (K + 1) / 2, tiles = (N + 31) / 32;
    for (int t = 0; t < tiles; t++)
        for (int s = 0; s < steps; s++)
            for (int l = 0; l < 64; l++) {
                const int k = 2 * s + (l >> 5), n = 32 * t + (l & 31);
                out[((int64_t)t * steps + s) * 64 + l] = (k < K && n < N) ? w[(int64_t)k * N + n] : 0.f;
            }
}

void pol::packBf16(const float *w, int K, int N, uint16_t *out)
{
    const int steps = (K + 15) / 16, tiles = (N + 31) / 32;
    for (int t = 0; t < tiles; t++)
        for (int s = 0; s < steps; s++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int k = 16 * s + 8 * (l >> 5) + j, n = 32 * t + (l & 31);
                    out[(((int64_t)t * steps + s) * 64 + l) * 8 + j] = (k < K && n < N) ? bf16Bits(w[(int64_t)k * N + n]) : 0;
                }
}

namespace {

struct Reader {
    std::string dir, err;
    int code = MPENV_OK;

    // One tensor file of the wanted shape (rank 1: d1 == 0).
    bool read(const std::string &name, int d0, int d1, std::vector<float> &out)
    {
        const std::string path = dir + "/" + name;
        auto bad = [&](int c, const std::string &why) {
            code = c;
            err = "policy checkpoint: " + path + ": " + why;
            return false;
        };
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f) return bad(MPENV_ERR_IO, "cannot open file");
        const int wantRank = d1 ? 2 : 1;
        int32_t ndim = 0, shape[2] = { 0, 0 };
        bool ok = std::fread(&ndim, sizeof(ndim), 1, f) == 1;
        if (ok && ndim != wantRank) {
            std::fclose(f);
            return bad(MPENV_ERR_INVALID, "wrong rank " + std::to_string(ndim) + ", expected " + std::to_string(wantRank));
        }
        ok = ok && std::fread(shape, sizeof(int32_t), (size_t)wantRank, f) == (size_t)wantRank;
        if (!ok) {
            std::fclose(f);
            return bad(MPENV_ERR_IO, "truncated file (header)");
        }
        if (shape[0] != d0 || shape[1] != d1) {
            std::fclose(f);
            std::string got = std::to_string(shape[0]), want = std::to_string(d0);
            if (d1) {
                got += " x " + std::to_string(shape[1]);
                want += " x " + std::to_string(d1);
            }
            return bad(MPENV_ERR_INVALID, "wrong shape " + got + ", expected " + want);
        }
        const size_t n = (size_t)d0 * (size_t)(d1 ? d1 : 1);
        out.resize(n);
        const size_t got = std::fread(out.data(), sizeof(float), n, f);
        std::fclose(f);
        if (got != n)
            return bad(MPENV_ERR_IO, "truncated file (" + std::to_string(got) + " of " + std::to_string(n) + " values)");
        return true;
    }
};

} // namespace

int policyRead(const char *dir, std::vector<float> *blob, std::string &err)
{
    using namespace pol;
    if (!dir) {
        err = "policy checkpoint: null directory";
        return MPENV_ERR_INVALID;
    }
    Reader r;
    r.dir = dir;
    const Layout L = layout();
    const LayoutBf16 B = layoutBf16();
    std::vector<float> out, t;
    if (blob) out.assign((size_t)B.total, 0.f);
    auto half = [&](int64_t at) { return reinterpret_cast<uint16_t *>(out.data() + at); };
    auto put = [&](int64_t at) {
        if (blob) std::memcpy(out.data() + at, t.data(), t.size() * sizeof(float));
    };

    // loadNormParams (dnn.cpp:1169-1360); element i of a mean / inverse-sigma
    // file belongs to element i of the observation it normalises
    static const struct { const char *name; int at, n; } kNorm[] = {
        { "self", kNormSelf, kSelfObs },          { "teammates", kNormTm, kOtherObs },
        { "opponents", kNormOpp, kOtherObs },     { "opponents_last_known", kNormLk, kOtherObs },
        { "fwd_lidar", kNormFwd, 4 },             { "rear_lidar", kNormRear, 4 },
        { "reward_coefs", kNormCoefs, kCoefs },
    };
    for (const auto &n : kNorm) {
        const std::string base = std::string("obs_preprocess_state_") + n.name;
        if (!r.read(base + "_mu", n.n, 0, t)) return err = r.err, r.code;
        put(L.normMean + n.at);
        if (!r.read(base + "_inv_sigma", n.n, 0, t)) return err = r.err, r.code;
        put(L.normInv + n.at);
    }

    // the embed modules, in the reference's file order (dnn.cpp:1367-1414)
    static const struct { const char *name; int mod, ln; } kEmb[] = {
        { "fwd_lidar", kModFwd, 0 },  { "rear_lidar", kModRear, 1 }, { "self", kModSelf, 2 },
        { "teammates", kModTm, 3 },   { "opponents", kModOpp, 4 },   { "opponents_last_known", kModLk, 5 },
    };
    for (const auto &e : kEmb) {
        const std::string ln = "params_backbone_prefix_LayerNorm_" + std::to_string(e.ln) + "_impl";
        if (!r.read(std::string("params_backbone_prefix_") + e.name + "_embed_kernel", kModIn[e.mod], kEmbed, t))
            return err = r.err, r.code;
        put(L.embedW[e.mod]);
        if (!r.read(ln + "_scale", kEmbed, 0, t)) return err = r.err, r.code;
        put(L.embedScale[e.mod]);
        if (!r.read(ln + "_bias", kEmbed, 0, t)) return err = r.err, r.code;
        put(L.embedBias[e.mod]);
    }

    // the trunk (dnn.cpp:1416-1429)
    for (int i = 0; i < 3; i++) {
        const std::string base = "params_backbone_actor_encoder_net_MaxPoolNet_0_MLP_0_";
        const int K = i == 0 ? kTrunkIn : kHidden;
        if (!r.read(base + "Dense_" + std::to_string(i) + "_kernel", K, kHidden, t)) return err = r.err, r.code;
        if (blob) {
            packB(t.data(), K, kHidden, out.data() + L.trunkW[i]);
            packBf16(t.data(), K, kHidden, half(B.trunkW[i]));
        }
        if (!r.read(base + "LayerNorm_" + std::to_string(i) + "_impl_scale", kHidden, 0, t)) return err = r.err, r.code;
        put(L.trunkScale[i]);
        if (!r.read(base + "LayerNorm_" + std::to_string(i) + "_impl_bias", kHidden, 0, t)) return err = r.err, r.code;
        put(L.trunkBias[i]);
    }

    // the two heads (dnn.cpp:1432-1437) as one [512][37] dense
    std::vector<float> heads((size_t)kHidden * kLogits);
    const int headN[2] = { kDiscreteLogits, kAimLogits };
    int col = 0;
    for (int h = 0; h < 2; h++) {
        const std::string base = "params_actor_DenseLayerDiscreteActor_" + std::to_string(h) + "_impl";
        if (!r.read(base + "_kernel", kHidden, headN[h], t)) return err = r.err, r.code;
        for (int k = 0; k < kHidden; k++)
            for (int n = 0; n < headN[h]; n++) heads[(size_t)k * kLogits + col + n] = t[(size_t)k * headN[h] + n];
        if (!r.read(base + "_bias", headN[h], 0, t)) return err = r.err, r.code;
        put(L.headBias + col);
        col += headN[h];
    }
    if (blob) {
        packB(heads.data(), kHidden, kLogits, out.data() + L.headW);
        packBf16(heads.data(), kHidden, kLogits, half(B.headW));
        blob->swap(out);
    }
    return MPENV_OK;
}

} // namespace mpenv
