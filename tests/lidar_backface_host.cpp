// Host side of tests/test_lidar_backface.py: built by the test with the host
// compiler against csrc/scene.cpp, it runs the product's octantNodeImages /
// octantBackFacing on a tree and rays the test hands over in a file and
// writes back what the test checks.
//
// The traversal below restates geom_dev.h bvhTraceRayT<false, kOctNodeQ,
// true, true> (k_lidar's and the LIDAR_RAY hook's configuration) on the
// host: the ray's octant image, near slab in qMin and far slab in qMax,
// fused slab products, slots in order until the array ends, internal
// children on a LIFO stack, and the watertight test of rayTri with its
// double fallback.  brute() runs the same triangle test over a plain list.
//
// input  (little endian): int32 mode, numNodes, numVerts, numRays;
//                         numNodes x 64 B nodes; numVerts x 3 f32;
//                         numRays x 3 f32 origins; numRays x 3 f32 directions
// output mode 0 (tree):   8 x numNodes nodes unpruned; 8 x numNodes pruned;
//                         t[numRays] f32, hit[numRays] i32 on the unpruned
//                         images; the same on the pruned images
// output mode 1 (soup):   dead[8][numVerts / 3] u8 (octantBackFacing);
//                         t, hit over all triangles; t, hit over the
//                         triangles alive in the ray's octant
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene.h"

using namespace mpenv;
using namespace mp;

namespace {

struct Txfm {
    int kx, ky, kz;
    float Sx, Sy, Sz;
};

Txfm rayTxfm(Vec3 d, Vec3 inv_d)
{
    const float ax = fabs_(d.x), ay = fabs_(d.y), az = fabs_(d.z);
    int kz;
    if (ax > ay && ax > az) kz = 0;
    else if (ay > az) kz = 1;
    else kz = 2;
    int kx = kz + 1; if (kx == 3) kx = 0;
    int ky = kx + 1; if (ky == 3) ky = 0;
    if (comp(d, kz) < 0.f) { int t = kx; kx = ky; ky = t; }
    Txfm t;
    t.kx = kx; t.ky = ky; t.kz = kz;
    t.Sx = comp(d, kx) * comp(inv_d, kz);
    t.Sy = comp(d, ky) * comp(inv_d, kz);
    t.Sz = comp(inv_d, kz);
    return t;
}

bool rayTri(Vec3 ta, Vec3 tb, Vec3 tc, const Txfm &tx, Vec3 org, float t_max, float &out_t)
{
    const Vec3 A = ta - org, B = tb - org, C = tc - org;
    const float Az_ = comp(A, tx.kz), Bz_ = comp(B, tx.kz), Cz_ = comp(C, tx.kz);
    const float Ax = fma_(-tx.Sx, Az_, comp(A, tx.kx));
    const float Ay = fma_(-tx.Sy, Az_, comp(A, tx.ky));
    const float Bx = fma_(-tx.Sx, Bz_, comp(B, tx.kx));
    const float By = fma_(-tx.Sy, Bz_, comp(B, tx.ky));
    const float Cx = fma_(-tx.Sx, Cz_, comp(C, tx.kx));
    const float Cy = fma_(-tx.Sy, Cz_, comp(C, tx.ky));
    float U = fma_(Cx, By, -(Cy * Bx));
    float V = fma_(Ax, Cy, -(Ay * Cx));
    float W = fma_(Bx, Ay, -(By * Ax));
    if (U < 0.0f || V < 0.0f || W < 0.0f) return false;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
        V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
        W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
        if (U < 0.0f || V < 0.0f || W < 0.0f) return false;
    }
    const float det = U + V + W;
    if (det == 0.f) return false;
    const float Az = tx.Sz * Az_, Bz = tx.Sz * Bz_, Cz = tx.Sz * Cz_;
    const float T = fma_(U, Az, fma_(V, Bz, W * Cz));
    if (T < 0.0f || T > t_max * det) return false;
    out_t = T * (1.0f / det);
    return true;
}

int rayOctant(Vec3 d)
{
    return (int)((f2u(d.x) >> 31) | ((f2u(d.y) >> 31) << 1) | ((f2u(d.z) >> 31) << 2));
}

float expScale(int8_t e) { return u2f((uint32_t)((int32_t)e + 127) << 23); }

// images: [8][n] nodes
bool traceOct(const BVHNode *images, size_t n, const std::vector<Vec3> &verts, Vec3 o, Vec3 d, float &t_out)
{
    const float diveps = 0.0000001f;
    const Vec3 inv_d = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
    const Txfm tx = rayTxfm(d, inv_d);
    const float rx = copysign_(d.x == 0 ? 1 / diveps : 1 / d.x, d.x);
    const float ry = copysign_(d.y == 0 ? 1 / diveps : 1 / d.y, d.y);
    const float rz = copysign_(d.z == 0 ? 1 / diveps : 1 / d.z, d.z);
    const BVHNode *nodes = images + (size_t)rayOctant(d) * n;
    float t_max = kFltMax;
    bool ray_hit = false;
    std::vector<int32_t> stack;
    stack.push_back(0);
    while (!stack.empty()) {
        const BVHNode &nd = nodes[stack.back()];
        stack.pop_back();
        const float dqx = expScale(nd.expX) * rx, dqy = expScale(nd.expY) * ry, dqz = expScale(nd.expZ) * rz;
        const float oqx = (nd.minX - o.x) * rx, oqy = (nd.minY - o.y) * ry, oqz = (nd.minZ - o.z) * rz;
        for (int i = 0; i < 4; i++) {
            const int32_t child = nd.children[i];
            if (child == -1) continue;
            const float nx = fma_((float)nd.qMinX[i], dqx, oqx), ny = fma_((float)nd.qMinY[i], dqy, oqy),
                        nz = fma_((float)nd.qMinZ[i], dqz, oqz);
            const float fx = fma_((float)nd.qMaxX[i], dqx, oqx), fy = fma_((float)nd.qMaxY[i], dqy, oqy),
                        fz = fma_((float)nd.qMaxZ[i], dqz, oqz);
            const float t_near = fmax_(fmax_(nx, ny), fmax_(nz, 0.f));
            const float t_far = fmin_(fmin_(fmin_(fx, fy), fz), t_max);
            if (!(t_near <= t_far)) continue;
            if (child & 0x80000000) {
                const int leaf = child & 0x7fffffff;
                bool hit_tri = false;
                float hit_t = 0.f, leaf_tmax = t_max;
                for (int k = 0; k < 2 && k < nd.triSize[i]; k++)
                    if (rayTri(verts[(leaf + k) * 3], verts[(leaf + k) * 3 + 1], verts[(leaf + k) * 3 + 2], tx, o,
                               leaf_tmax, hit_t)) {
                        hit_tri = true;
                        leaf_tmax = hit_t;
                    }
                if (hit_tri) {
                    ray_hit = true;
                    t_max = hit_t;
                }
            } else {
                stack.push_back(child);
            }
        }
    }
    t_out = t_max;
    return ray_hit;
}

// every triangle in order, each accepted hit tightening t_max; dead: skip mask or null
bool brute(const std::vector<Vec3> &verts, const uint8_t *dead, Vec3 o, Vec3 d, float &t_out)
{
    const Txfm tx = rayTxfm(d, v3(1.f / d.x, 1.f / d.y, 1.f / d.z));
    float t_max = kFltMax, t = 0.f;
    bool hit = false;
    for (size_t k = 0; k < verts.size() / 3; k++) {
        if (dead && dead[k]) continue;
        if (rayTri(verts[3 * k], verts[3 * k + 1], verts[3 * k + 2], tx, o, t_max, t)) {
            hit = true;
            t_max = t;
        }
    }
    t_out = t_max;
    return hit;
}

template <typename T> void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hdr[4];
    if (fread(hdr, 4, 4, in) != 4) return 2;
    const int mode = hdr[0];
    const size_t n = hdr[1], nv = hdr[2], nr = hdr[3];
    std::vector<BVHNode> nodes(n);
    std::vector<Vec3> verts(nv), org(nr), dir(nr);
    if (fread(nodes.data(), 64, n, in) != n || fread(verts.data(), 12, nv, in) != nv ||
        fread(org.data(), 12, nr, in) != nr || fread(dir.data(), 12, nr, in) != nr)
        return 2;
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    std::vector<float> t0(nr), t1(nr);
    std::vector<int32_t> h0(nr), h1(nr);
    if (mode == 0) {
        const std::vector<BVHNode> full = octantNodeImages(nodes), pruned = octantNodeImages(nodes, verts, true);
        for (size_t r = 0; r < nr; r++) {
            h0[r] = traceOct(full.data(), n, verts, org[r], dir[r], t0[r]);
            h1[r] = traceOct(pruned.data(), n, verts, org[r], dir[r], t1[r]);
        }
        put(out, full);
        put(out, pruned);
    } else {
        const size_t nt = nv / 3;
        std::vector<uint8_t> dead(8 * nt);
        for (int oct = 0; oct < 8; oct++)
            for (size_t k = 0; k < nt; k++)
                dead[oct * nt + k] = octantBackFacing(verts[3 * k], verts[3 * k + 1], verts[3 * k + 2], oct);
        for (size_t r = 0; r < nr; r++) {
            h0[r] = brute(verts, nullptr, org[r], dir[r], t0[r]);
            h1[r] = brute(verts, dead.data() + (size_t)rayOctant(dir[r]) * nt, org[r], dir[r], t1[r]);
        }
        put(out, dead);
    }
    put(out, t0);
    put(out, h0);
    put(out, t1);
    put(out, h1);
    fclose(out);
    return 0;
}
