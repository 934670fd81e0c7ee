// A caller written against Manager::Config::maps and Manager::numMaps /
// mapInfo (include/mpenv_manager.hpp): member pointers, so a missing or
// mistyped declaration fails to compile; then, without a GPU, a list the
// engine refuses before it touches the device throws with the refusal's words.
// Built and run by tests/test_maps.py.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mpenv_manager.hpp"

using namespace madronaMPEnv;

template <typename T> static void use(T) {}

int main(int argc, char **argv)
{
    use<int (Manager::*)() const>(&Manager::numMaps);
    use<Manager::MapInfo (Manager::*)(int) const>(&Manager::mapInfo);
    const std::string scene = argc > 1 ? argv[1] : "scenes/simple_map";

    Manager::Config cfg {};
    cfg.execMode = ExecMode::CUDA;
    cfg.numWorlds = 5;
    cfg.randSeed = 5;
    cfg.autoReset = true;
    cfg.taskType = Task::Zone;
    cfg.teamSize = 3;
    cfg.maps = { { scene, 2 }, { scene, 2 } }; // four worlds, not five
    try {
        Manager mgr(cfg);
        std::fprintf(stderr, "a map set whose counts do not sum to numWorlds was accepted\n");
        return 1;
    } catch (const std::runtime_error &e) {
        if (!std::strstr(e.what(), "4 worlds") || !std::strstr(e.what(), "num_worlds is 5")) {
            std::fprintf(stderr, "unexpected refusal: %s\n", e.what());
            return 1;
        }
    }
    std::printf("maps caller ok\n");
    return 0;
}
