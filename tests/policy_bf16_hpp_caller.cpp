// A caller written against include/mpenv_manager.hpp that switches the
// precision of in-sim policy inference: F32 by default, BF16 set before the
// load and honoured by it, switched between steps without a reload, and a
// value that is neither refused with both names.  Built and run by
// tests/test_policy_bf16_gpu.py:  policy_bf16_caller SCENE_DIR WEIGHTS_DIR
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mpenv_manager.hpp"

using namespace madronaMPEnv;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
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
        Manager mgr(cfg);
        if (mgr.policyPrecision() != MPENV_POLICY_F32) throw std::runtime_error("the default precision is not F32");
        mgr.setPolicyPrecision(MPENV_POLICY_BF16);
        mgr.loadPolicy(argv[2]);
        if (mgr.policyPrecision() != MPENV_POLICY_BF16) throw std::runtime_error("the load changed the precision");
        mgr.init();
        for (int i = 0; i < 3; i++) mgr.step();
        mgr.setPolicyPrecision(MPENV_POLICY_F32);
        mgr.step();
        if (mgr.policyPrecision() != MPENV_POLICY_F32 || !mgr.policyLoaded())
            throw std::runtime_error("the switch back to F32 did not hold");
        try {
            mgr.setPolicyPrecision(7);
            throw std::runtime_error("precision 7 was accepted");
        } catch (const std::exception &e) {
            if (!strstr(e.what(), "MPENV_POLICY_F32") || !strstr(e.what(), "MPENV_POLICY_BF16")) throw;
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "unexpected: %s\n", e.what());
        return 1;
    }
    printf("policy bf16 caller ok\n");
    return 0;
}
