// A caller written against include/mpenv_manager.hpp that sets
// Manager::Config::policyWeightsPath (src/mgr.hpp:49): the checkpoint is
// loaded by the constructor and steps run with it; a directory that does not
// load makes the constructor throw with the file named.  Built and run by
// tests/test_policy_gpu.py:  policy_caller SCENE_DIR WEIGHTS_DIR MISSING_DIR
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mpenv_manager.hpp"

using namespace madronaMPEnv;

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
        cfg.policyWeightsPath = argv[2];
        Manager mgr(cfg);
        if (!mgr.policyLoaded()) throw std::runtime_error("policyWeightsPath was ignored");
        mgr.init();
        for (int i = 0; i < 3; i++) mgr.step();
        mgr.unloadPolicy();
        if (mgr.policyLoaded()) throw std::runtime_error("unloadPolicy left the policy loaded");
        mgr.loadPolicy(argv[2]);
        mgr.step();
    } catch (const std::exception &e) {
        fprintf(stderr, "unexpected: %s\n", e.what());
        return 1;
    }
    try {
        cfg.policyWeightsPath = argv[3];
        Manager mgr(cfg);
        fprintf(stderr, "a missing checkpoint directory was accepted\n");
        return 1;
    } catch (const std::exception &e) {
        if (!strstr(e.what(), "cannot open") || !strstr(e.what(), "obs_preprocess_state_self_mu")) {
            fprintf(stderr, "wrong message: %s\n", e.what());
            return 1;
        }
    }
    printf("policy caller ok\n");
    return 0;
}
