// A caller written against include/mpenv_manager.hpp that runs a league: one
// checkpoint per policy id (loadPolicy(dir, id), unloadPolicy(id),
// policySlots, policyForward(..., id)), next to the one-checkpoint calls,
// which keep their meaning.  Built and run by tests/test_policy_slots_gpu.py:
//   policy_slots_caller SCENE_DIR WEIGHTS_DIR_A WEIGHTS_DIR_B
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mpenv_manager.hpp"

using namespace madronaMPEnv;

static void expect(bool ok, const char *what)
{
    if (!ok) throw std::runtime_error(what);
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string scene = argv[1];
    const std::string col = scene + "/collisions.bin", nav = scene + "/navmesh.bin", spw = scene + "/spawns.bin",
                      zon = scene + "/zones.bin";
    Manager::Config cfg {};
    cfg.execMode = ExecMode::CUDA;
    cfg.gpuID = 0;
    cfg.numWorlds = 3;
    cfg.randSeed = 5;
    cfg.autoReset = true;
    cfg.simFlags = SimFlags::Default;
    cfg.taskType = Task::Zone;
    cfg.teamSize = 2;
    cfg.numPBTPolicies = 0;
    cfg.policyHistorySize = 1;
    cfg.map = { scene.c_str(), col.c_str(), nav.c_str(), spw.c_str(), zon.c_str(), Vector3::zero(), 0.f };
    try {
        cfg.policyWeightsPath = argv[2]; // policy id 0
        Manager mgr(cfg);
        expect(mgr.policySlots() == std::vector<int> { 0 }, "policyWeightsPath did not load policy id 0");
        mgr.init();
        mgr.loadPolicy(argv[3], 3);
        mgr.loadPolicy(argv[3], MPENV_POLICY_SLOTS - 1);
        expect(mgr.policySlots() == std::vector<int> { 0, 3, 31 }, "loadPolicy(dir, id) missed its id");
        mgr.setAgentPolicy(0, 1, AgentPolicy { 3 });
        mgr.setAgentPolicy(1, 0, AgentPolicy { 31 });
        mgr.setAgentPolicy(2, 2, AgentPolicy { 9 }); // empty: served by id 0
        for (int i = 0; i < 3; i++) mgr.step();
        mgr.loadPolicy(argv[2], 3); // hot swap
        mgr.step();
        mgr.unloadPolicy(3);
        expect(mgr.policySlots() == std::vector<int> { 0, 31 } && mgr.policyLoaded(), "unloadPolicy(id) missed its id");
        mgr.step();
        float *const notRead = reinterpret_cast<float *>(uintptr_t(256)); // refused before any launch
        try {
            mgr.policyForward(notRead, nullptr, nullptr, 3);
            expect(false, "policyForward through an empty id was accepted");
        } catch (const std::runtime_error &e) {
            expect(strstr(e.what(), "slot 3 is empty") != nullptr, e.what());
        }
        try {
            mgr.loadPolicy(argv[2], MPENV_POLICY_SLOTS);
            expect(false, "a policy id past the last slot was accepted");
        } catch (const std::runtime_error &e) {
            expect(strstr(e.what(), "[0, 32)") != nullptr, e.what());
        }
        mgr.unloadPolicy();
        expect(mgr.policySlots().empty() && !mgr.policyLoaded(), "unloadPolicy() left a checkpoint loaded");
        mgr.loadPolicy(argv[2]);
        expect(mgr.policySlots() == std::vector<int> { 0 }, "loadPolicy(dir) is policy id 0");
        mgr.step();
    } catch (const std::exception &e) {
        fprintf(stderr, "unexpected: %s\n", e.what());
        return 1;
    }
    printf("policy slots caller ok\n");
    return 0;
}
