// manager_scene.cpp — the scene's two ways out of the host: the device image
// mpenv_create uploads (buildSceneDev) and the GPU-free mpenv_scene_* queries
// that tests and the oracle read.  What both derive from a Scene is derived
// by one function here.
#include <cstring>

#include "manager.h"

namespace {

// The quirk guard of k_move's sphere casts (scene.h quirkGrid): the cast
// radius is always consts::agentRadius.
QuirkGrid sceneQuirkGrid(const Scene &s)
{
    return quirkGrid(s.bvhVerts, 15.f, 2.f, 16.f);
}

// The navmesh de-indexed: 9 floats (3 vertices) per triangle into `out`.
void navTriVerts(const NavMesh &nm, float *out)
{
    for (size_t t = 0; t < nm.numTris(); t++)
        for (int k = 0; k < 3; k++) {
            const mp::Vec3 v = nm.verts[nm.tris[3 * t + k]];
            out[9 * t + 3 * k + 0] = v.x;
            out[9 * t + 3 * k + 1] = v.y;
            out[9 * t + 3 * k + 2] = v.z;
        }
}

// The counts the LDS-size functions of engine.h read, without device pointers.
SceneDev sceneCounts(const Scene &s)
{
    SceneDev sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.numNodes = (int32_t)s.nodes.size();
    sc.numVerts = (int32_t)s.bvhVerts.size();
    sc.numLidarNodes = (int32_t)s.lidarNodes.size();
    sc.numLidarVerts = (int32_t)s.lidarVerts.size();
    sc.numA = (int32_t)s.aSpawns.size();
    sc.numB = (int32_t)s.bSpawns.size();
    sc.numCommon = (int32_t)s.commonRespawns.size();
    return sc;
}

// A BVH query's answer: the counts always, nodes and vertices where the
// caller's buffer is there and its capacity (the count passed in) suffices.
void bvhOut(const std::vector<BVHNode> &nodes, const std::vector<mp::Vec3> &verts, int32_t maxStack, void *nodes_out,
            int32_t *num_nodes, float *verts_out, int32_t *num_verts, int32_t *max_stack)
{
    if (num_nodes) {
        if (nodes_out && *num_nodes >= (int32_t)nodes.size())
            std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(BVHNode));
        *num_nodes = (int32_t)nodes.size();
    }
    if (num_verts) {
        if (verts_out && *num_verts >= (int32_t)verts.size()) std::memcpy(verts_out, verts.data(), verts.size() * 12);
        *num_verts = (int32_t)verts.size();
    }
    if (max_stack) *max_stack = maxStack;
}

} // namespace

// Path selection.  LDS-resident: node indices fit the byte stack's entries,
// the stack bounds its 16 entries, and each step kernel's dynamic LDS request
// the 64 KB a block gets without a function attribute.  Global-resident: the
// stack bounds fit the WideStack (as many entries as the oracle's stack), the
// triangles k_vis's 16-bit occluder hints, and what k_sim and k_vis still
// keep in LDS the same 64 KB.
SceneLimits mpenv::sceneLimits(const Scene &s)
{
    SceneLimits l;
    l.tris = (int32_t)(s.bvhVerts.size() / 3);
    l.lidarTris = (int32_t)(s.lidarVerts.size() / 3);
    l.nodes = (int32_t)s.nodes.size();
    l.lidarNodes = (int32_t)s.lidarNodes.size();
    l.stack = std::max(s.maxStack, s.maxStackAnyOrder);
    l.lidarStack = s.lidarMaxStack;
    const SceneDev sc = sceneCounts(s);
    l.ldsMove = moveLdsBytes(sc, kResidencyLds);
    l.ldsSim = simLdsBytes(sc, kResidencyLds);
    l.ldsVis = visLdsBytes(sc, kResidencyLds, 0);
    l.ldsLidar = lidarLdsBytes(sc, kResidencyLds);
    l.globalBytes = bvhLdsBytesSphere(sc) + bvhLdsBytesOct(sc);
    auto num = [](size_t v) { return std::to_string(v); };
    if (l.nodes > kMaxLdsNodes) l.ldsWhyNot = "collision BVH has " + num(l.nodes) + " nodes (byte stack: 256)";
    else if (l.lidarNodes > kMaxLdsNodes) l.ldsWhyNot = "lidar BVH has " + num(l.lidarNodes) + " nodes (byte stack: 256)";
    else if (l.stack > kMaxBVHStack) l.ldsWhyNot = "collision BVH stack bound " + num(l.stack) + " (register stack: 16)";
    else if (l.lidarStack > kMaxBVHStack) l.ldsWhyNot = "lidar BVH stack bound " + num(l.lidarStack) + " (register stack: 16)";
    else if (l.ldsMove > kLdsBudget) l.ldsWhyNot = "k_move would ask for " + num(l.ldsMove) + " B of LDS (64 KB)";
    else if (l.ldsSim > kLdsBudget) l.ldsWhyNot = "k_sim would ask for " + num(l.ldsSim) + " B of LDS (64 KB)";
    else if (l.ldsVis > kLdsBudget) l.ldsWhyNot = "k_vis would ask for " + num(l.ldsVis) + " B of LDS (64 KB)";
    else if (l.ldsLidar > kLdsBudget) l.ldsWhyNot = "k_lidar would ask for " + num(l.ldsLidar) + " B of LDS (64 KB)";
    l.ldsOk = l.ldsWhyNot.empty();
    if (l.tris > kMaxSceneTris)
        l.reason = num(l.tris) + " collision triangles (k_vis's 16-bit occluder hints: " + num(kMaxSceneTris) + ")";
    else if (l.stack > kMaxGlobalStack)
        l.reason = "collision BVH stack bound " + num(l.stack) + " (traversal stack: " + num(kMaxGlobalStack) + ")";
    else if (l.lidarStack > kMaxGlobalStack)
        l.reason = "lidar BVH stack bound " + num(l.lidarStack) + " (traversal stack: " + num(kMaxGlobalStack) + ")";
    else if (!l.ldsOk && simLdsBytes(sc, kResidencyGlobal) > kLdsBudget)
        l.reason = "spawn lists need " + num(simLdsBytes(sc, kResidencyGlobal)) + " B of k_sim's LDS (64 KB)";
    l.supported = l.reason.empty();
    return l;
}

// What buildSceneDev refuses for the task and flags, decided from the host
// scene alone (mpenv_maps_plan answers without a GPU).
std::string mpenv::sceneTaskProblem(const Scene &s, const mpenv_config &cfg)
{
    if (s.zoneAABBs.empty() || s.zoneAABBs.size() > (size_t)kMaxZones) return "bad zone count";
    if (s.numDefaultASpawns == 0 || s.numDefaultBSpawns == 0) return "scene needs A and B spawns";
    if ((cfg.sim_flags & MPENV_SIMFLAG_SPAWN_IN_MIDDLE) &&
        (s.aSpawns.size() == s.numDefaultASpawns || s.bSpawns.size() == s.numDefaultBSpawns))
        // the reference would index past its spawn array here (utils.cpp:358-366)
        return "SpawnInMiddle: no free middle cells in this scene";
    // initWorld starts every ZoneCaptureDefend episode at zone 3 (sim.cpp:822-825)
    if (cfg.task_type == MPENV_TASK_ZONE_CAPTURE_DEFEND && s.zoneAABBs.size() < 4)
        return "ZoneCaptureDefend needs a scene with >= 4 zones";
    // sub-zones 0 and 1 are zones 1 and 2 (level_gen.cpp:283-293)
    if ((cfg.sim_flags & MPENV_SIMFLAG_SUB_ZONES) && s.zoneAABBs.size() < 3) return "SubZones needs a scene with >= 3 zones";
    return "";
}

void mpenv::buildSceneDev(mpenv_manager &m, const Scene &s, const SceneLimits &limits, SceneDev &sc, SceneImages &img)
{
    std::memset(&sc, 0, sizeof(sc));
    if (!limits.supported) throw std::runtime_error("scene not supported: " + limits.reason);
    if (const std::string why = sceneTaskProblem(s, m.cfg); !why.empty()) throw std::runtime_error(why);

    BVHNode *d_nodes = m.alloc<BVHNode>(s.nodes.size());
    m.upload(d_nodes, s.nodes.data(), sizeof(BVHNode) * s.nodes.size());
    {
        // k_lidar: octant images of the lidar tree, each without the
        // triangles its octant's rays can only meet from behind, and the
        // tree's triangles
        const std::vector<BVHNode> oct = octantNodeImages(s.lidarNodes, s.lidarVerts, true);
        BVHNode *d_oct = m.alloc<BVHNode>(oct.size());
        m.upload(d_oct, oct.data(), sizeof(BVHNode) * oct.size());
        sc.octNodes = d_oct;
        float *d_lv = m.alloc<float>(s.lidarVerts.size() * 3);
        m.upload(d_lv, s.lidarVerts.data(), sizeof(float) * 3 * s.lidarVerts.size());
        sc.lidarVerts = d_lv;
        sc.numLidarNodes = (int32_t)s.lidarNodes.size();
        sc.numLidarVerts = (int32_t)s.lidarVerts.size();
    }
    float *d_verts = m.alloc<float>(s.bvhVerts.size() * 3);
    m.upload(d_verts, s.bvhVerts.data(), sizeof(float) * 3 * s.bvhVerts.size());
    auto upSpawns = [&](const std::vector<Spawn> &v) {
        Spawn *p = m.alloc<Spawn>(std::max<size_t>(v.size(), 1));
        if (!v.empty()) m.upload(p, v.data(), sizeof(Spawn) * v.size());
        return p;
    };
    {
        const NavMesh &nm = s.nav;
        const size_t T = nm.numTris();
        std::vector<float> tv(std::max<size_t>(T * 9, 1), 0.f);
        navTriVerts(nm, tv.data());
        float *d_nav = m.alloc<float>(tv.size());
        m.upload(d_nav, tv.data(), sizeof(float) * tv.size());
        int32_t *d_astar = m.alloc<int32_t>(std::max<size_t>(nm.astar.size(), 1));
        if (!nm.astar.empty()) m.upload(d_astar, nm.astar.data(), sizeof(int32_t) * nm.astar.size());
        std::vector<float> cdf(std::max<size_t>(T, 1), 0.f);
        mp::navAreaCDF(tv.data(), (int)T, cdf.data());
        float *d_cdf = m.alloc<float>(cdf.size());
        m.upload(d_cdf, cdf.data(), sizeof(float) * cdf.size());
        sc.navCdf = d_cdf;
        sc.navTris = d_nav;
        sc.astar = d_astar;
        sc.numNavTris = (int32_t)T;
    }
    {
        // sphere-cast triangle constants (geom_dev.h sphereTriD)
        const size_t nt = s.bvhVerts.size() / 3;
        std::vector<float> pre(std::max<size_t>(nt, 1) * 8, 0.f);
        for (size_t t = 0; t < nt; t++) {
            const mp::Vec3 a = s.bvhVerts[3 * t], b = s.bvhVerts[3 * t + 1], c = s.bvhVerts[3 * t + 2];
            const mp::Vec3 e01 = b - a, e02 = c - a, e12 = c - b;
            const mp::Vec3 nu = mp::computeTriangleGeoNormal(e01, e02, e12);
            const float n_len = mp::length(nu);
            const mp::Vec3 n = nu / n_len;
            float *o = &pre[8 * t];
            o[0] = n.x; o[1] = n.y; o[2] = n.z; o[3] = n_len;
            o[4] = mp::length2(e01); o[5] = mp::length2(e02); o[6] = mp::length2(e12); o[7] = 0.f;
        }
        float *d_pre = m.alloc<float>(pre.size());
        m.upload(d_pre, pre.data(), sizeof(float) * pre.size());
        sc.triPre = d_pre;
    }
    {
        const QuirkGrid q = sceneQuirkGrid(s);
        uint32_t *d_q = m.alloc<uint32_t>(std::max<size_t>(q.bits.size(), 1));
        if (!q.bits.empty()) m.upload(d_q, q.bits.data(), sizeof(uint32_t) * q.bits.size());
        sc.quirkGrid = d_q;
        sc.qgMinX = q.minX;
        sc.qgMinY = q.minY;
        sc.qgInvCell = 1.f / q.cell;
        sc.qgW = q.w;
        sc.qgH = q.h;
    }
    sc.nodes = d_nodes;
    sc.verts = d_verts;
    sc.numNodes = (int32_t)s.nodes.size();
    sc.numVerts = (int32_t)s.bvhVerts.size();
    sc.worldBounds = s.worldBounds;
    // sim.cpp:5855 maxDist; 5869-5882 frustumData
    sc.maxDist = mp::length(s.worldBounds.pMax - s.worldBounds.pMin);
    {
        float aspect = 16.f / 9.f;
        float ang = 90.f / 2.f * (mp::kPi / 180.f);
        float f = 1.f / (mp::sinf_(ang) / mp::cosf_(ang));
        float wx = f / aspect, wy = 1.f, hx = f, hy = 1.f;
        float wi = 1.f / mp::sqrt_(wx * wx + wy * wy);
        float hi = 1.f / mp::sqrt_(hx * hx + hy * hy);
        sc.frustum[0] = wx * wi; sc.frustum[1] = wy * wi;
        sc.frustum[2] = hx * hi; sc.frustum[3] = hy * hi;
    }
    sc.aSpawns = upSpawns(s.aSpawns);
    sc.bSpawns = upSpawns(s.bSpawns);
    sc.commonRespawns = upSpawns(s.commonRespawns);
    sc.numA = (int32_t)s.aSpawns.size();
    sc.numB = (int32_t)s.bSpawns.size();
    sc.numCommon = (int32_t)s.commonRespawns.size();
    sc.numDefaultA = (int32_t)s.numDefaultASpawns;
    sc.numDefaultB = (int32_t)s.numDefaultBSpawns;
    sc.spawnTrackLen = (int32_t)std::max<size_t>(
        kMinSpawnTrack, std::max(s.aSpawns.size(), std::max(s.bSpawns.size(), s.commonRespawns.size())));
    sc.numZones = (int32_t)s.zoneAABBs.size();
    sc.task = m.cfg.task_type;
    sc.flank = m.cfg.train_flank ? 1 : 0; // RewardMode::Flank applies to Task.Zone (sim.cpp:5733-5748)
    if (m.cfg.curriculum_data_path) {
        // mgr.cpp:1424-1441: the file is an array of CurriculumSnapshot
        // (size / 176 of them).  Snapshots naming a zone or controller the
        // scene does not have are rejected (the reference would index past
        // its zone arrays).
        FILE *f = std::fopen(m.cfg.curriculum_data_path, "rb");
        if (!f) throw IoError(std::string("cannot open curriculum data ") + m.cfg.curriculum_data_path);
        std::fseek(f, 0, SEEK_END);
        const long size = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        std::vector<mpenv_curriculum_snapshot> snaps((size_t)std::max<long>(size, 0) / sizeof(mpenv_curriculum_snapshot));
        const size_t got = snaps.empty() ? 0 : std::fread(snaps.data(), sizeof(mpenv_curriculum_snapshot), snaps.size(), f);
        std::fclose(f);
        if (got != snaps.size()) throw std::runtime_error("short read of curriculum data");
        for (const mpenv_curriculum_snapshot &sn : snaps) {
            if (sn.cur_zone >= s.zoneAABBs.size() || sn.cur_zone_controller < -1 || sn.cur_zone_controller > 1)
                throw std::runtime_error("curriculum snapshot names a zone or controller outside the scene");
        }
        if (!snaps.empty()) {
            auto *d = m.alloc<mpenv_curriculum_snapshot>(snaps.size());
            m.upload(d, snaps.data(), sizeof(mpenv_curriculum_snapshot) * snaps.size());
            sc.curriculum = d;
        }
        sc.numSnapshots = (int32_t)snaps.size();
    }
    if (m.cfg.sim_flags & MPENV_SIMFLAG_SUB_ZONES) {
        mp::subZoneTable(s.zoneAABBs.data(), s.zoneRotations.data(), sc.subZones);
    }
    for (int z = 0; z < sc.numZones; z++) {
        sc.zoneAABB[z] = s.zoneAABBs[z];
        sc.zoneRot[z] = s.zoneRotations[z];
    }
    for (int z = 0; z < kMaxZones; z++) sc.zoneGoalTri[z] = -1;
    if (sc.numNavTris > 0)
        launched(computeZoneGoalTris(sc, m.alloc<int32_t>(kMaxZones), sc.zoneGoalTri, m.stream),
                 "zone goal triangle kernel failed");
    sc.numGoals = (int32_t)s.goalRegions.size();
    for (int gi = 0; gi < sc.numGoals && gi < 4; gi++) {
        const GoalRegion &g = s.goalRegions[gi];
        GoalRegionDev &d = sc.goals[gi];
        for (int k = 0; k < 3; k++) {
            d.sub[k].pMin = g.subRegions[k].pMin;
            d.sub[k].pMax = g.subRegions[k].pMax;
            d.sub[k].rotation = g.subRegions[k].rotation;
        }
        d.numSub = g.numSubRegions;
        d.attackerTeam = g.attackerTeam;
        d.rewardStrength = g.rewardStrength;
    }
    {
        SceneTables t;
        std::memcpy(t.zoneAABB, sc.zoneAABB, sizeof(t.zoneAABB));
        std::memcpy(t.zoneRot, sc.zoneRot, sizeof(t.zoneRot));
        std::memcpy(t.subZones, sc.subZones, sizeof(t.subZones));
        std::memcpy(t.goals, sc.goals, sizeof(t.goals));
        std::memcpy(t.zoneGoalTri, sc.zoneGoalTri, sizeof(t.zoneGoalTri));
        SceneTables *d_tab = m.alloc<SceneTables>(1);
        m.upload(d_tab, &t, sizeof(t));
        launched(computeSceneFrames(d_tab, m.stream), "k_scene_frames launch failed");
        sc.tab = d_tab;
    }
    {
        // the global-resident images, whichever path is in use: switching
        // residency later allocates nothing
        img.sphere = m.alloc<char>(bvhLdsBytesSphere(sc));
        img.oct = m.alloc<char>(bvhLdsBytesOct(sc));
        img.residency = limits.ldsOk ? kResidencyLds : kResidencyGlobal;
        launched(buildSceneImages(sc, img, m.stream), "k_scene_images launch failed");
    }
    sc.simFlags = m.cfg.sim_flags;
    sc.autoReset = m.cfg.auto_reset;
    sc.worldOffset = m.cfg.world_id_offset;
    // mgr.cpp:1736-1737
    sc.initRandKey = mp::splitI(mp::initKey(m.cfg.rand_seed), 0);
}

// Map sets: the list as mpenv_create_maps will hold it.  Every refusal names
// the range index and its directory.  Equal paths load once.
int mpenv::planMaps(const mpenv_config &cfg, const mpenv_map_range *maps, int32_t n, MapPlan &plan, mpenv_map_desc *desc)
{
    if (desc)
        for (int32_t r = 0; r < n && r < MPENV_MAX_MAP_RANGES; r++) std::memset(&desc[r], 0, sizeof(desc[r]));
    if (cfg.scene_path) return fail(MPENV_ERR_INVALID, "map set: scene_path must be null when a map list is given");
    if (n < 1 || n > MPENV_MAX_MAP_RANGES)
        return fail(MPENV_ERR_INVALID, "map set: " + std::to_string(n) + " ranges (1 to " +
                                           std::to_string(MPENV_MAX_MAP_RANGES) + ")");
    auto where = [&](int32_t r) {
        return "map range " + std::to_string(r) + " (" + (maps[r].scene_path ? maps[r].scene_path : "null") + ")";
    };
    uint64_t sum = 0;
    for (int32_t r = 0; r < n; r++) {
        if (!maps[r].scene_path) return fail(MPENV_ERR_INVALID, where(r) + ": scene_path is null");
        if (maps[r].num_worlds == 0) return fail(MPENV_ERR_INVALID, where(r) + ": a range needs at least one world");
        sum += maps[r].num_worlds;
    }
    if (sum != cfg.num_worlds)
        return fail(MPENV_ERR_INVALID, "map set: the ranges hold " + std::to_string(sum) + " worlds, num_worlds is " +
                                           std::to_string(cfg.num_worlds));
    int rc = MPENV_OK;
    std::string firstWhy;
    int32_t w0 = 0;
    for (int32_t r = 0; r < n; r++) {
        const std::string path = maps[r].scene_path;
        size_t si = 0;
        while (si < plan.scenes.size() && plan.scenes[si].path != path) si++;
        if (si == plan.scenes.size()) {
            MapScene ms;
            ms.path = path;
            try {
                ms.scene = loadScene(path, (cfg.sim_flags & MPENV_SIMFLAG_SPAWN_IN_MIDDLE) != 0);
            } catch (const std::exception &e) {
                return fail(MPENV_ERR_IO, where(r) + ": " + e.what());
            }
            ms.limits = sceneLimits(ms.scene);
            ms.collisionsHash = fnv1a64File(path + "/collisions.bin");
            plan.scenes.push_back(std::move(ms));
        }
        const MapScene &ms = plan.scenes[si];
        std::string why = ms.limits.supported ? sceneTaskProblem(ms.scene, cfg) : "scene not supported: " + ms.limits.reason;
        if (desc) {
            desc[r].first_world = w0;
            desc[r].num_worlds = (int32_t)maps[r].num_worlds;
            desc[r].scene = (int32_t)si;
            desc[r].supported = why.empty() ? 1 : 0;
            desc[r].residency = !why.empty() ? MPENV_SCENE_AUTO : ms.limits.ldsOk ? MPENV_SCENE_LDS : MPENV_SCENE_GLOBAL;
            std::snprintf(desc[r].reason, sizeof(desc[r].reason), "%s", why.empty() ? ms.limits.ldsWhyNot.c_str() : why.c_str());
        }
        if (!why.empty() && rc == MPENV_OK) {
            rc = MPENV_ERR_INVALID;
            firstWhy = where(r) + ": " + why;
        }
        MapRange mr;
        mr.scene = (int32_t)si;
        mr.w0 = w0;
        mr.n = (int32_t)maps[r].num_worlds;
        plan.ranges.push_back(mr);
        w0 += mr.n;
        const Scene &s = ms.scene;
        plan.spawnTrackLen = (int32_t)std::max<size_t>(
            { (size_t)plan.spawnTrackLen, (size_t)kMinSpawnTrack, s.aSpawns.size(), s.bSpawns.size(), s.commonRespawns.size() });
    }
    return rc == MPENV_OK ? MPENV_OK : fail(rc, firstWhy);
}

// The queries below load the scene themselves and touch no GPU; whatever
// the load throws is an I/O error to their callers.
extern "C" {

int mpenv_maps_plan(const mpenv_config *cfg, const mpenv_map_range *maps, int32_t n, mpenv_map_desc *out,
                    int32_t *spawn_track_len)
{
    if (!cfg || !maps) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&]() -> int {
        MapPlan plan;
        const int rc = planMaps(*cfg, maps, n, plan, out);
        if (spawn_track_len) *spawn_track_len = plan.spawnTrackLen;
        return rc;
    }, MPENV_ERR_INVALID);
}

// Host-side access to the navmesh and A* table (tests / oracle input).
int mpenv_scene_navmesh(const char *scene_path, float *tri_verts_out, int32_t *num_tris, int32_t *adj_out,
                        int32_t *astar_out)
{
    return guarded([&] {
        const Scene s = loadScene(scene_path);
        const NavMesh &nm = s.nav;
        if (!num_tris) return;
        if (*num_tris >= (int32_t)nm.numTris()) {
            if (tri_verts_out) navTriVerts(nm, tri_verts_out);
            if (adj_out) std::memcpy(adj_out, nm.adj.data(), sizeof(int32_t) * 3 * nm.numTris());
            if (astar_out) std::memcpy(astar_out, nm.astar.data(), sizeof(int32_t) * nm.astar.size());
        }
        *num_tris = (int32_t)nm.numTris();
    }, MPENV_ERR_IO);
}

// The quirk guard k_move uploads (for tests).
int mpenv_scene_quirk_grid(const char *scene_path, int32_t *header_out, uint32_t *bits_out, int32_t *num_words)
{
    if (!num_words) return fail(MPENV_ERR_INVALID, "num_words is null");
    return guarded([&] {
        const QuirkGrid q = sceneQuirkGrid(loadScene(scene_path));
        if (header_out) {
            std::memcpy(&header_out[0], &q.minX, 4);
            std::memcpy(&header_out[1], &q.minY, 4);
            std::memcpy(&header_out[2], &q.cell, 4);
            header_out[3] = q.w;
            header_out[4] = q.h;
        }
        if (bits_out && *num_words >= (int32_t)q.bits.size()) std::memcpy(bits_out, q.bits.data(), q.bits.size() * 4);
        *num_words = (int32_t)q.bits.size();
    }, MPENV_ERR_IO);
}

int mpenv_scene_info(const char *scene_path, mpenv_scene_info_t *out)
{
    if (!scene_path || !out) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        const SceneLimits l = sceneLimits(loadScene(scene_path));
        std::memset(out, 0, sizeof(*out));
        out->triangles = l.tris;
        out->collision_nodes = l.nodes;
        out->collision_stack = l.stack;
        out->lidar_nodes = l.lidarNodes;
        out->lidar_stack = l.lidarStack;
        out->lidar_triangles = l.lidarTris;
        out->supported = l.supported ? 1 : 0;
        out->residency = !l.supported ? MPENV_SCENE_AUTO : l.ldsOk ? MPENV_SCENE_LDS : MPENV_SCENE_GLOBAL;
        out->lds_bytes_move = (int64_t)l.ldsMove;
        out->lds_bytes_sim = (int64_t)l.ldsSim;
        out->lds_bytes_vis = (int64_t)l.ldsVis;
        out->lds_bytes_lidar = (int64_t)l.ldsLidar;
        out->global_bytes = (int64_t)l.globalBytes;
        std::snprintf(out->reason, sizeof(out->reason), "%s", l.supported ? l.ldsWhyNot.c_str() : l.reason.c_str());
    }, MPENV_ERR_IO);
}

// Host-side access to the scene BVH (for the parity oracle and tests).
int mpenv_scene_bvh_variant(const char *scene_path, const int32_t *opts, int32_t num_opts, void *nodes_out,
                            int32_t *num_nodes, float *verts_out, int32_t *num_verts, int32_t *max_stack)
{
    return guarded([&] {
        const Scene s = loadScene(scene_path);
        BVHBuildOpts o;
        if (opts && num_opts > 0) o.maxLeaf = opts[0];
        if (opts && num_opts > 1) o.bins = opts[1];
        if (opts && num_opts > 2) o.measure = opts[2];
        if (opts && num_opts > 3) o.travCost = (float)opts[3] / 100.f;
        if (opts && num_opts > 4) o.floorWeight = (float)opts[4] / 100.f;
        for (int32_t k = 5; opts && k + 1 < num_opts; k += 2) {
            if (opts[k] >= 0) o.splitRank[(uint64_t)opts[k]] = opts[k + 1];
            else o.collapseChoice[(uint64_t)(-(int64_t)opts[k])] = opts[k + 1];
        }
        Scene t;
        buildBVH(s.triVerts, t, o);
        bvhOut(t.nodes, t.bvhVerts, std::max(t.maxStack, t.maxStackAnyOrder), nodes_out, num_nodes, verts_out,
               num_verts, max_stack);
    }, MPENV_ERR_IO);
}

int mpenv_scene_lidar_bvh(const char *scene_path, void *nodes_out, int32_t *num_nodes, float *verts_out,
                          int32_t *num_verts, int32_t *max_stack)
{
    return guarded([&] {
        const Scene s = loadScene(scene_path);
        bvhOut(s.lidarNodes, s.lidarVerts, s.lidarMaxStack, nodes_out, num_nodes, verts_out, num_verts, max_stack);
    }, MPENV_ERR_IO);
}

int mpenv_scene_bvh(const char *scene_path, void *nodes_out, int32_t *num_nodes, float *verts_out,
                    int32_t *num_verts, int32_t *max_stack)
{
    return guarded([&] {
        const Scene s = loadScene(scene_path);
        bvhOut(s.nodes, s.bvhVerts, std::max(s.maxStack, s.maxStackAnyOrder), nodes_out, num_nodes, verts_out,
               num_verts, max_stack);
    }, MPENV_ERR_IO);
}

} // extern "C"
