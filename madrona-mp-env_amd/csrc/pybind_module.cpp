// pybind_module.cpp — the `madrona_mp_env` Python module (reference:
// src/bindings.cpp:11-160, nanobind; nanobind is absent, pybind11 is used).
//
// Same names, enum values and SimManager.__init__ keyword arguments as the
// reference, layered over the C ABI of include/mpenv.h.  Tensor getters
// return zero-copy views of engine-owned device memory; .to_torch() hands
// them to PyTorch through DLPack (kDLROCM), like madrona::py::Tensor
// (mgr.cpp:295-301, 655-661).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "mpenv.h"

namespace py = pybind11;

namespace {

// ---- minimal DLPack ABI (dlpack.h v0.8)
struct DLDevice { int32_t device_type; int32_t device_id; };
struct DLDataType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor {
    void *data;
    DLDevice device;
    int32_t ndim;
    DLDataType dtype;
    int64_t *shape;
    int64_t *strides;
    uint64_t byte_offset;
};
struct DLManagedTensor {
    DLTensor dl_tensor;
    void *manager_ctx;
    void (*deleter)(DLManagedTensor *self);
};
constexpr int32_t kDLCPU = 1;
constexpr int32_t kDLROCM = 10;

struct ManagerHandle {
    mpenv_manager *mgr = nullptr;
    ~ManagerHandle()
    {
        if (mgr) mpenv_destroy(mgr);
    }
};

void check(int rc)
{
    if (rc != MPENV_OK) throw std::runtime_error(std::string("madrona_mp_env: ") + mpenv_last_error());
}

struct PyTensor {
    std::shared_ptr<ManagerHandle> owner;
    void *ptr = nullptr;
    int32_t dtype = MPENV_DTYPE_FLOAT32;
    std::vector<int64_t> dims;
    int32_t gpu = -1;

    struct Ctx {
        std::shared_ptr<ManagerHandle> owner;
        std::vector<int64_t> shape;
    };

    py::capsule dlpack() const
    {
        auto *mt = new DLManagedTensor();
        auto *ctx = new Ctx { owner, dims };
        mt->dl_tensor.data = ptr;
        mt->dl_tensor.device = { gpu >= 0 ? kDLROCM : kDLCPU, gpu >= 0 ? gpu : 0 };
        mt->dl_tensor.ndim = (int32_t)dims.size();
        // kDLInt 0, kDLUInt 1, kDLFloat 2; the camera's label image is the one 8-bit tensor, the
        // league's standings table the one 64-bit (signed) one
        uint8_t code = dtype == MPENV_DTYPE_FLOAT32 ? 2 : (dtype == MPENV_DTYPE_UINT32 || dtype == MPENV_DTYPE_UINT8 ? 1 : 0);
        mt->dl_tensor.dtype = { code, (uint8_t)(dtype == MPENV_DTYPE_UINT8 ? 8 : dtype == MPENV_DTYPE_INT64 ? 64 : 32), 1 };
        mt->dl_tensor.shape = ctx->shape.data();
        mt->dl_tensor.strides = nullptr;
        mt->dl_tensor.byte_offset = 0;
        mt->manager_ctx = ctx;
        mt->deleter = [](DLManagedTensor *self) {
            delete static_cast<Ctx *>(self->manager_ctx);
            delete self;
        };
        return py::capsule(mt, "dltensor", [](PyObject *cap) {
            if (PyCapsule_IsValid(cap, "dltensor")) {
                auto *m = static_cast<DLManagedTensor *>(PyCapsule_GetPointer(cap, "dltensor"));
                if (m && m->deleter) m->deleter(m);
            }
        });
    }
};

struct PySimManager {
    std::shared_ptr<ManagerHandle> h;

    PyTensor tensor(int32_t id) const
    {
        PyTensor t;
        t.owner = h;
        int32_t ndim = 0;
        int64_t dims[8];
        check(mpenv_export_tensor(h->mgr, id, &t.ptr, &t.dtype, &ndim, dims, &t.gpu));
        t.dims.assign(dims, dims + ndim);
        return t;
    }

    // the camera's depth (MPENV_CAMERA_DEPTH) or label image (mpenv_camera.h)
    PyTensor cameraTensor(int32_t which) const
    {
        PyTensor t;
        t.owner = h;
        int32_t ndim = 0;
        int64_t dims[8];
        check(mpenv_camera_tensor(h->mgr, which, &t.ptr, &t.dtype, &ndim, dims, &t.gpu));
        t.dims.assign(dims, dims + ndim);
        return t;
    }

    // the league's table, weights or draws (mpenv_league.h)
    PyTensor leagueTensor(int32_t which) const
    {
        PyTensor t;
        t.owner = h;
        int32_t ndim = 0;
        int64_t dims[8];
        check(mpenv_league_tensor(h->mgr, which, &t.ptr, &t.dtype, &ndim, dims, &t.gpu));
        t.dims.assign(dims, dims + ndim);
        return t;
    }

    // the curriculum pool or its ticks (mpenv_curriculum.h)
    PyTensor poolTensor(int32_t which) const
    {
        PyTensor t;
        t.owner = h;
        int32_t ndim = 0;
        int64_t dims[8];
        check(mpenv_curriculum_pool_tensor(h->mgr, which, &t.ptr, &t.dtype, &ndim, dims, &t.gpu));
        t.dims.assign(dims, dims + ndim);
        return t;
    }
};

// step_range None: the whole episode, (0, episode_len - 1)
constexpr int32_t kPyEpisodeLen = 3000; // consts.hpp episodeLen
mpenv_curriculum_pool_config poolConfigOf(int32_t capacity, int32_t period, const py::object &step_range, uint32_t need,
                                          uint32_t seed)
{
    int32_t lo = 0, hi = kPyEpisodeLen - 1;
    if (!step_range.is_none()) {
        const auto r = step_range.cast<std::pair<int32_t, int32_t>>();
        lo = r.first;
        hi = r.second;
    }
    return { capacity, period, lo, hi, need, seed };
}

// "none" / "team1" / "both" <-> MPENV_LEAGUE_DRAW_*
const char *const kLeagueDrawNames[] = { "none", "team1", "both" };
int32_t leagueDrawOf(const std::string &name)
{
    for (int32_t k = 0; k < 3; k++)
        if (name == kLeagueDrawNames[k]) return k;
    throw py::value_error("draw must be \"none\", \"team1\" or \"both\"");
}

// Unscoped so that pybind11 generates |, &, ^ (sim_flags |= SimFlags.X,
// scripts/jax_train.py:80-100).
enum SimFlagsE : uint32_t {
    SimFlagsE_Default = 0,
    SimFlagsE_SpawnInMiddle = 1u << 0,
    SimFlagsE_RandomizeHPMagazine = 1u << 1,
    SimFlagsE_NavmeshSpawn = 1u << 2,
    SimFlagsE_NoRespawn = 1u << 3,
    SimFlagsE_StaggerStarts = 1u << 4,
    SimFlagsE_EnableCurriculum = 1u << 5,
    SimFlagsE_HardcodedSpawns = 1u << 6,
    SimFlagsE_RandomFlipTeams = 1u << 7,
    SimFlagsE_StaticFlipTeams = 1u << 8,
    SimFlagsE_FullTeamPolicy = 1u << 9,
    SimFlagsE_SimEvalMode = 1u << 10,
    SimFlagsE_SubZones = 1u << 11,
};

// scene_path as a map set (mpenv_maps.h): a sequence of (directory, number of
// worlds); `paths` keeps the strings the ranges point into.
std::vector<mpenv_map_range> mapRanges(const py::object &list, std::vector<std::string> &paths)
{
    for (py::handle item : list) {
        const py::sequence pair = py::reinterpret_borrow<py::sequence>(item);
        if (py::len(pair) != 2) throw py::value_error("a map set is a list of (scene directory, number of worlds)");
        paths.push_back(py::str(pair[0]));
    }
    std::vector<mpenv_map_range> ranges;
    size_t k = 0;
    for (py::handle item : list) {
        const py::sequence pair = py::reinterpret_borrow<py::sequence>(item);
        ranges.push_back({ paths[k++].c_str(), pair[1].cast<uint32_t>() });
    }
    return ranges;
}

const char *residencyName(int32_t mode) { return mode == MPENV_SCENE_LDS ? "lds" : "global"; }

// The flat buffer array of gpuStreamInit / gpuStreamStep: exactly one
// pointer per trainInterface input and output (the C ABI reads that many).
std::vector<void *> streamBuffers(const std::vector<uintptr_t> &bufs)
{
    int32_t ni = 0, no = 0;
    mpenv_train_interface_size(&ni, &no);
    if (bufs.size() != (size_t)(ni + no))
        throw py::value_error("gpu_stream_*: buffers must hold " + std::to_string(ni + no) +
                              " pointers (trainInterface inputs then outputs), got " + std::to_string(bufs.size()));
    std::vector<void *> b(bufs.size());
    for (size_t k = 0; k < bufs.size(); k++) b[k] = reinterpret_cast<void *>(bufs[k]);
    return b;
}

} // namespace

PYBIND11_MODULE(madrona_mp_env, m)
{
    m.doc() = "MI355X-native madrona-mp-env engine (Zone task, gfx950 HIP kernels)";

    // madrona.ExecMode submodule (madrona::py::setupMadronaSubmodule)
    py::module_ madrona = m.def_submodule("madrona", "madrona runtime enums");
    enum class ExecMode : int32_t { CPU = MPENV_EXEC_CPU, CUDA = MPENV_EXEC_CUDA };
    py::enum_<ExecMode>(madrona, "ExecMode").value("CPU", ExecMode::CPU).value("CUDA", ExecMode::CUDA);

    enum class Task : uint32_t { Explore = 0, TDM = 1, Zone = 2, Turret = 3, ZoneCaptureDefend = 4 };
    py::enum_<Task>(m, "Task")
        .value("Explore", Task::Explore)
        .value("TDM", Task::TDM)
        .value("Zone", Task::Zone)
        .value("Turret", Task::Turret)
        .value("ZoneCaptureDefend", Task::ZoneCaptureDefend);

    py::enum_<SimFlagsE>(m, "SimFlags", py::arithmetic())
        .value("Default", SimFlagsE_Default)
        .value("SpawnInMiddle", SimFlagsE_SpawnInMiddle)
        .value("RandomizeHPMagazine", SimFlagsE_RandomizeHPMagazine)
        .value("NavmeshSpawn", SimFlagsE_NavmeshSpawn)
        .value("NoRespawn", SimFlagsE_NoRespawn)
        .value("StaggerStarts", SimFlagsE_StaggerStarts)
        .value("EnableCurriculum", SimFlagsE_EnableCurriculum)
        .value("HardcodedSpawns", SimFlagsE_HardcodedSpawns)
        .value("RandomFlipTeams", SimFlagsE_RandomFlipTeams)
        .value("StaticFlipTeams", SimFlagsE_StaticFlipTeams)
        .value("FullTeamPolicy", SimFlagsE_FullTeamPolicy)
        .value("SimEvalMode", SimFlagsE_SimEvalMode)
        .value("SubZones", SimFlagsE_SubZones);

    py::class_<PyTensor>(m, "Tensor")
        .def_property_readonly("shape", [](const PyTensor &t) { return py::tuple(py::cast(t.dims)); })
        .def_property_readonly("dtype", [](const PyTensor &t) {
            return t.dtype == MPENV_DTYPE_FLOAT32  ? "float32"
                   : t.dtype == MPENV_DTYPE_UINT32 ? "uint32"
                   : t.dtype == MPENV_DTYPE_UINT8  ? "uint8"
                   : t.dtype == MPENV_DTYPE_INT64  ? "int64"
                                                   : "int32";
        })
        .def_property_readonly("gpu_id", [](const PyTensor &t) { return t.gpu; })
        .def("data_ptr", [](const PyTensor &t) { return reinterpret_cast<uintptr_t>(t.ptr); })
        .def("__dlpack__", [](const PyTensor &t, py::object) { return t.dlpack(); }, py::arg("stream") = py::none())
        .def("__dlpack_device__", [](const PyTensor &t) {
            return py::make_tuple(t.gpu >= 0 ? kDLROCM : kDLCPU, t.gpu >= 0 ? t.gpu : 0);
        })
        .def("to_torch", [](const PyTensor &t) {
            py::object from_dlpack = py::module_::import("torch.utils.dlpack").attr("from_dlpack");
            return from_dlpack(t.dlpack());
        });

    // "f32" / "bf16" <-> MPENV_POLICY_F32 / MPENV_POLICY_BF16
    auto precision_of = [](const std::string &name) -> int32_t {
        if (name == "f32") return MPENV_POLICY_F32;
        if (name == "bf16") return MPENV_POLICY_BF16;
        throw std::invalid_argument("policy precision must be \"f32\" or \"bf16\", not \"" + name + "\"");
    };

    py::class_<PySimManager>(m, "SimManager")
        .def(py::init([precision_of](ExecMode exec_mode, int64_t gpu_id, int64_t num_worlds, int64_t rand_seed, bool auto_reset,
                         uint32_t sim_flags, Task task, uint32_t team_size, uint32_t num_pbt_policies,
                         uint32_t policy_history_size, py::object scene_path, bool train_flank,
                         py::object replay_log_path, py::object record_log_path, py::object event_log_path,
                         py::object curriculum_data_path, uint32_t world_id_offset,
                         py::object policy_weights_path, const std::string &policy_precision) {
                 const int32_t precision = precision_of(policy_precision);
                 std::string replay, record, event, curric, weights, scene;
                 // a str: one scene directory; a list of (directory, worlds): a map set (mpenv_maps.h)
                 std::vector<std::string> map_paths;
                 std::vector<mpenv_map_range> ranges;
                 const bool map_set = !py::isinstance<py::str>(scene_path);
                 if (map_set) ranges = mapRanges(scene_path, map_paths);
                 else scene = py::str(scene_path);
                 mpenv_config cfg = {};
                 cfg.exec_mode = (int32_t)exec_mode;
                 cfg.gpu_id = (int32_t)gpu_id;
                 cfg.num_worlds = (uint32_t)num_worlds;
                 cfg.rand_seed = (uint32_t)rand_seed;
                 cfg.auto_reset = auto_reset ? 1 : 0;
                 cfg.sim_flags = sim_flags;
                 cfg.task_type = (int32_t)task;
                 cfg.team_size = team_size;
                 cfg.num_pbt_policies = num_pbt_policies;
                 cfg.policy_history_size = policy_history_size;
                 cfg.scene_path = map_set ? nullptr : scene.c_str();
                 cfg.train_flank = train_flank ? 1 : 0;
                 if (!replay_log_path.is_none()) { replay = py::str(replay_log_path); cfg.replay_log_path = replay.c_str(); }
                 if (!record_log_path.is_none()) { record = py::str(record_log_path); cfg.record_log_path = record.c_str(); }
                 if (!event_log_path.is_none()) { event = py::str(event_log_path); cfg.event_log_path = event.c_str(); }
                 if (!curriculum_data_path.is_none()) {
                     curric = py::str(curriculum_data_path);
                     cfg.curriculum_data_path = curric.c_str();
                 }
                 cfg.world_id_offset = world_id_offset;
                 auto h = std::make_shared<ManagerHandle>();
                 {
                     py::gil_scoped_release nogil;
                     check(map_set ? mpenv_create_maps(&cfg, ranges.data(), (int32_t)ranges.size(), &h->mgr)
                                   : mpenv_create(&cfg, &h->mgr));
                 }
                 check(mpenv_policy_set_precision(h->mgr, precision));
                 // Manager::Config::policyWeightsPath (mgr.hpp:49): loaded after the create, failing loudly;
                 // a {policy_id: dir} dict loads one checkpoint per id (mpenv_policy_slots.h)
                 if (py::isinstance<py::dict>(policy_weights_path)) {
                     for (auto item : policy_weights_path.cast<py::dict>()) {
                         weights = py::str(item.second);
                         check(mpenv_policy_load_slot(h->mgr, item.first.cast<int32_t>(), weights.c_str()));
                     }
                 } else if (!policy_weights_path.is_none()) {
                     weights = py::str(policy_weights_path);
                     check(mpenv_policy_load(h->mgr, weights.c_str()));
                 }
                 return PySimManager { h };
             }),
             py::arg("exec_mode"), py::arg("gpu_id"), py::arg("num_worlds"), py::arg("rand_seed"),
             py::arg("auto_reset"), py::arg("sim_flags"), py::arg("task_type"), py::arg("team_size"),
             py::arg("num_pbt_policies"), py::arg("policy_history_size"), py::arg("scene_path"),
             py::arg("train_flank") = false, py::arg("replay_log_path") = py::none(),
             py::arg("record_log_path") = py::none(), py::arg("event_log_path") = py::none(),
             py::arg("curriculum_data_path") = py::none(), py::arg("world_id_offset") = 0,
             py::arg("policy_weights_path") = py::none(), py::arg("policy_precision") = "f32")
        .def("init", [](PySimManager &s) { py::gil_scoped_release nogil; check(mpenv_init(s.h->mgr)); })
        .def("step", [](PySimManager &s) { py::gil_scoped_release nogil; check(mpenv_step(s.h->mgr)); })
        .def("step_async", [](PySimManager &s, uintptr_t stream) {
            check(mpenv_step_async(s.h->mgr, reinterpret_cast<void *>(stream)));
        }, py::arg("stream") = 0)
        .def("copy_actions", [](PySimManager &s, uintptr_t src, uintptr_t stream) {
            check(mpenv_copy_actions(s.h->mgr, reinterpret_cast<const int32_t *>(src), reinterpret_cast<void *>(stream)));
        }, py::arg("src"), py::arg("stream") = 0)
        .def("combat_actions", [](PySimManager &s, uintptr_t tape, uintptr_t out, int32_t mode, uintptr_t stream) {
            check(mpenv_combat_actions(s.h->mgr, reinterpret_cast<const int32_t *>(tape),
                                       reinterpret_cast<int32_t *>(out), mode, reinterpret_cast<void *>(stream)));
        }, py::arg("tape"), py::arg("out") = 0, py::arg("mode") = 1, py::arg("stream") = 0)
        // Manager::gpuStreamInit / gpuStreamStep (mgr.cpp:507-645): the flat
        // buffer array of the XLA custom call -- trainInterface inputs then
        // outputs, caller-owned device pointers (0 = skip that tensor).
        .def("gpu_stream_init", [](PySimManager &s, uintptr_t stream, const std::vector<uintptr_t> &bufs) {
            std::vector<void *> b = streamBuffers(bufs);
            check(mpenv_gpu_stream_init(s.h->mgr, reinterpret_cast<void *>(stream), b.data()));
        }, py::arg("stream"), py::arg("buffers"))
        .def("gpu_stream_step", [](PySimManager &s, uintptr_t stream, const std::vector<uintptr_t> &bufs) {
            std::vector<void *> b = streamBuffers(bufs);
            check(mpenv_gpu_stream_step(s.h->mgr, reinterpret_cast<void *>(stream), b.data()));
        }, py::arg("stream"), py::arg("buffers"))
        // the learner exchange's compact wire format (include/mpenv.h
        // mpenv_wire_*): sizes, pack into / unpack from device buffers
        .def("wire_bytes", [](PySimManager &s, bool keyframe) {
            int64_t b = 0;
            check(mpenv_wire_bytes(s.h->mgr, keyframe ? 1 : 0, &b));
            return b;
        }, py::arg("keyframe") = false)
        .def("wire_pack", [](PySimManager &s, uintptr_t dst, bool keyframe, uintptr_t stream) {
            check(mpenv_wire_pack(s.h->mgr, reinterpret_cast<void *>(dst), keyframe ? 1 : 0,
                                  reinterpret_cast<void *>(stream)));
        }, py::arg("dst"), py::arg("keyframe") = false, py::arg("stream") = 0)
        .def("wire_unpack", [](PySimManager &s, uintptr_t src, bool keyframe, uintptr_t stream) {
            check(mpenv_wire_unpack(s.h->mgr, reinterpret_cast<const void *>(src), keyframe ? 1 : 0,
                                    reinterpret_cast<void *>(stream)));
        }, py::arg("src"), py::arg("keyframe") = false, py::arg("stream") = 0)
        .def("wire_error", [](PySimManager &s) {
            uint32_t e = 0;
            check(mpenv_wire_error(s.h->mgr, &e));
            return e;
        })
        .def("wire_error_async", [](PySimManager &s, uintptr_t out, uintptr_t stream) {
            check(mpenv_wire_error_async(s.h->mgr, reinterpret_cast<uint32_t *>(out), reinterpret_cast<void *>(stream)));
        }, py::arg("out"), py::arg("stream"))
        // in-sim policy inference (include/mpenv.h mpenv_policy_*): logits
        // [A][37] f32 and actions [A][6] i32 are device pointers as integers
        // policy_id: the checkpoint slot (mpenv_policy_slots.h); unload_policy() empties every slot
        .def("load_policy", [](PySimManager &s, const std::string &dir, int32_t policy_id) {
            check(mpenv_policy_load_slot(s.h->mgr, policy_id, dir.c_str()));
        }, py::arg("dir"), py::arg("policy_id") = 0)
        .def("unload_policy", [](PySimManager &s, py::object policy_id) {
            check(policy_id.is_none() ? mpenv_policy_unload(s.h->mgr)
                                      : mpenv_policy_unload_slot(s.h->mgr, policy_id.cast<int32_t>()));
        }, py::arg("policy_id") = py::none())
        // "f32" (bit-equal to the reference) or "bf16" (trunk and heads on the bf16 matrix cores)
        .def("set_policy_precision", [precision_of](PySimManager &s, const std::string &name) {
            check(mpenv_policy_set_precision(s.h->mgr, precision_of(name)));
        }, py::arg("precision"))
        .def("policy_precision", [](PySimManager &s) {
            int32_t p = 0;
            check(mpenv_policy_precision(s.h->mgr, &p));
            return std::string(p == MPENV_POLICY_BF16 ? "bf16" : "f32");
        })
        .def("policy_slots", [](PySimManager &s) {
            uint32_t mask = 0;
            check(mpenv_policy_slots(s.h->mgr, &mask));
            std::vector<int> ids;
            for (int i = 0; i < MPENV_POLICY_SLOTS; i++)
                if ((mask >> i) & 1u) ids.push_back(i);
            return ids;
        })
        .def("policy_loaded", [](PySimManager &s) {
            int32_t on = 0;
            check(mpenv_policy_loaded(s.h->mgr, &on));
            return on != 0;
        })
        .def("policy_forward", [](PySimManager &s, uintptr_t logits, uintptr_t actions, uintptr_t stream,
                                  int32_t policy_id) {
            check(mpenv_policy_forward_slot(s.h->mgr, policy_id, reinterpret_cast<float *>(logits),
                                            reinterpret_cast<int32_t *>(actions), reinterpret_cast<void *>(stream)));
        }, py::arg("logits"), py::arg("actions") = 0, py::arg("stream") = 0, py::arg("policy_id") = 0)
        // world checkpoints (include/mpenv.h mpenv_state_*): device pointers
        // as integers, 0 = no world map / the manager's own stream
        .def("state_bytes", [](PySimManager &s) {
            int64_t b = 0;
            check(mpenv_state_bytes(s.h->mgr, &b));
            return b;
        })
        .def("state_dims", [](PySimManager &s) {
            uint32_t w = 0, t = 0, l = 0;
            check(mpenv_state_dims(s.h->mgr, &w, &t, &l));
            return py::make_tuple(w, t, l);
        })
        .def("save_state", [](PySimManager &s, uintptr_t dst, uintptr_t stream) {
            check(mpenv_state_save(s.h->mgr, reinterpret_cast<void *>(dst), reinterpret_cast<void *>(stream)));
        }, py::arg("dst"), py::arg("stream") = 0)
        .def("load_state", [](PySimManager &s, uintptr_t src, uintptr_t world_map, uintptr_t stream) {
            check(mpenv_state_load(s.h->mgr, reinterpret_cast<const void *>(src),
                                   reinterpret_cast<const int32_t *>(world_map), reinterpret_cast<void *>(stream)));
        }, py::arg("src"), py::arg("world_map") = 0, py::arg("stream") = 0)
        .def("state_error", [](PySimManager &s) {
            uint32_t e = 0;
            check(mpenv_state_error(s.h->mgr, &e));
            return e;
        })
        .def("set_world_groups", [](PySimManager &s, int32_t g) { check(mpenv_set_world_groups(s.h->mgr, g)); })
        // "auto", "lds" or "global" (mpenv_scene_residency.h); "lds" on a scene that does not fit raises
        .def("set_scene_residency", [](PySimManager &s, const std::string &name) {
            const int32_t mode = name == "auto" ? MPENV_SCENE_AUTO : name == "lds" ? MPENV_SCENE_LDS
                                 : name == "global"                               ? MPENV_SCENE_GLOBAL
                                                                                  : -1;
            check(mpenv_set_scene_residency(s.h->mgr, mode));
        }, py::arg("residency"))
        // the path in use: "lds" or "global"
        .def("scene_residency", [](PySimManager &s) {
            int32_t mode = 0;
            check(mpenv_scene_residency(s.h->mgr, &mode));
            return std::string(mode == MPENV_SCENE_LDS ? "lds" : "global");
        })
        // map sets (mpenv_maps.h): the ranges as the engine holds them (one for a single-map manager), and
        // the range index of every world as a zero-copy int32 [W]: the engine's own table, to be read only
        .def("maps", [](PySimManager &s) {
            int32_t n = 0;
            check(mpenv_num_maps(s.h->mgr, &n));
            py::list out;
            for (int32_t r = 0; r < n; r++) {
                mpenv_map_desc d;
                const char *path = nullptr;
                check(mpenv_map_info(s.h->mgr, r, &d, &path));
                out.append(py::dict(py::arg("path") = std::string(path ? path : ""), py::arg("first_world") = d.first_world,
                                    py::arg("num_worlds") = d.num_worlds, py::arg("scene") = d.scene,
                                    py::arg("residency") = residencyName(d.residency)));
            }
            return out;
        })
        .def("world_map_tensor", [](PySimManager &s) {
            PyTensor t;
            t.owner = s.h;
            t.dtype = MPENV_DTYPE_INT32;
            check(mpenv_map_of_world(s.h->mgr, &t.ptr));
            int32_t w = 0, n = 0;
            check(mpenv_dims(s.h->mgr, &w, &n));
            t.dims = { w };
            int32_t nd = 0, dt = 0;
            int64_t dims[8];
            void *unused = nullptr;
            check(mpenv_export_tensor(s.h->mgr, MPENV_EXPORT_RESET, &unused, &dt, &nd, dims, &t.gpu)); // the device id
            return t;
        })
        // the egocentric depth camera (mpenv_camera.h): per agent a [height][width] depth (float32) and
        // label (uint8: 0 nothing, 1 map, 2 teammate, 3 opponent) image, rendered behind every step and
        // init while enabled, and by render_camera() from the current state
        .def("enable_camera", [](PySimManager &s, int32_t width, int32_t height, float hfov_deg) {
            const mpenv_camera_config c { width, height, hfov_deg, 0 };
            check(mpenv_camera_enable(s.h->mgr, &c));
        }, py::arg("width"), py::arg("height"), py::arg("hfov_deg") = 90.0f)
        .def("disable_camera", [](PySimManager &s) { check(mpenv_camera_disable(s.h->mgr)); })
        // (width, height, hfov_deg), or None while disabled
        .def("camera_config", [](PySimManager &s) -> py::object {
            mpenv_camera_config c {};
            int32_t on = 0;
            check(mpenv_camera_enabled(s.h->mgr, &c, &on));
            if (!on) return py::none();
            return py::make_tuple(c.width, c.height, c.hfov_deg);
        })
        .def("render_camera", [](PySimManager &s, uintptr_t stream) {
            py::gil_scoped_release nogil;
            check(mpenv_camera_render(s.h->mgr, reinterpret_cast<void *>(stream)));
        }, py::arg("stream") = 0)
        .def("camera_depth", [](PySimManager &s) { return s.cameraTensor(MPENV_CAMERA_DEPTH); })
        .def("camera_label", [](PySimManager &s) { return s.cameraTensor(MPENV_CAMERA_LABEL); })
        // the league scheduler (mpenv_league.h): standings int64 [P+1, P+1, 8] and, by draw mode, a
        // weighted redraw of the policy ids of every world that ends an episode, behind every step and init
        .def("enable_league", [](PySimManager &s, int32_t num_policies, const std::string &draw, uint32_t seed) {
            const mpenv_league_config c { num_policies, leagueDrawOf(draw), seed, 0 };
            check(mpenv_league_enable(s.h->mgr, &c));
        }, py::arg("num_policies"), py::arg("draw") = "team1", py::arg("seed") = 0)
        .def("disable_league", [](PySimManager &s) { check(mpenv_league_disable(s.h->mgr)); })
        // (num_policies, draw, seed), or None while disabled
        .def("league_config", [](PySimManager &s) -> py::object {
            mpenv_league_config c {};
            int32_t on = 0;
            check(mpenv_league_enabled(s.h->mgr, &c, &on));
            if (!on) return py::none();
            return py::make_tuple(c.num_policies, std::string(kLeagueDrawNames[c.draw]), c.seed);
        })
        .def("league_table", [](PySimManager &s) { return s.leagueTensor(MPENV_LEAGUE_TABLE); })
        .def("league_weights", [](PySimManager &s) { return s.leagueTensor(MPENV_LEAGUE_WEIGHTS); })
        .def("league_draws", [](PySimManager &s) { return s.leagueTensor(MPENV_LEAGUE_DRAWS); })
        .def("clear_league", [](PySimManager &s, uintptr_t stream) {
            check(mpenv_league_clear(s.h->mgr, reinterpret_cast<void *>(stream)));
        }, py::arg("stream") = 0)
        .def("set_league_weights", [](PySimManager &s, py::array_t<int32_t, py::array::c_style | py::array::forcecast> w) {
            mpenv_league_config c {};
            int32_t on = 0;
            check(mpenv_league_enabled(s.h->mgr, &c, &on));
            if (on && w.size() != (py::ssize_t)(c.num_policies + 1) * c.num_policies)
                throw py::value_error("set_league_weights: weights must be [num_policies + 1, num_policies]");
            check(mpenv_league_set_weights(s.h->mgr, w.data()));
        }, py::arg("weights"))
        // the live curriculum pool (mpenv_curriculum.h): [R, capacity] snapshots in device memory that
        // episode starts read in place, refreshed behind every step from the running batch
        .def("enable_curriculum_pool", [](PySimManager &s, int32_t capacity, int32_t period, py::object step_range,
                                          uint32_t need, uint32_t seed) {
            const mpenv_curriculum_pool_config c = poolConfigOf(capacity, period, step_range, need, seed);
            check(mpenv_curriculum_pool_enable(s.h->mgr, &c));
        }, py::arg("capacity"), py::arg("period") = 64, py::arg("step_range") = py::none(), py::arg("need") = 0,
             py::arg("seed") = 0)
        .def("disable_curriculum_pool", [](PySimManager &s) { check(mpenv_curriculum_pool_disable(s.h->mgr)); })
        // capacity stays; an argument left None keeps its value
        .def("configure_curriculum_pool", [](PySimManager &s, py::object period, py::object step_range, py::object need,
                                             py::object seed) {
            mpenv_curriculum_pool_config c {};
            int32_t on = 0;
            check(mpenv_curriculum_pool_enabled(s.h->mgr, &c, &on));
            if (!period.is_none()) c.period = period.cast<int32_t>();
            if (!step_range.is_none()) {
                const auto r = step_range.cast<std::pair<int32_t, int32_t>>();
                c.step_lo = r.first;
                c.step_hi = r.second;
            }
            if (!need.is_none()) c.need = need.cast<uint32_t>();
            if (!seed.is_none()) c.seed = seed.cast<uint32_t>();
            if (!on) c.capacity = 1; // a valid configuration, so that the refusal names the disabled pool
            check(mpenv_curriculum_pool_configure(s.h->mgr, &c));
        }, py::arg("period") = py::none(), py::arg("step_range") = py::none(), py::arg("need") = py::none(),
             py::arg("seed") = py::none())
        // dict(capacity, period, step_range, need, seed), or None while disabled
        .def("curriculum_pool_config", [](PySimManager &s) -> py::object {
            mpenv_curriculum_pool_config c {};
            int32_t on = 0;
            check(mpenv_curriculum_pool_enabled(s.h->mgr, &c, &on));
            if (!on) return py::none();
            return py::dict(py::arg("capacity") = c.capacity, py::arg("period") = c.period,
                            py::arg("step_range") = py::make_tuple(c.step_lo, c.step_hi), py::arg("need") = c.need,
                            py::arg("seed") = c.seed);
        })
        // zero-copy: uint8 [R, capacity, 176] and uint32 [R, capacity]
        .def("curriculum_pool", [](PySimManager &s) { return s.poolTensor(MPENV_CURRICULUM_POOL); })
        .def("curriculum_pool_ticks", [](PySimManager &s) { return s.poolTensor(MPENV_CURRICULUM_TICKS); })
        .def("curriculum_pool_tick", [](PySimManager &s) {
            uint32_t t = 0;
            check(mpenv_curriculum_pool_tick(s.h->mgr, &t));
            return t;
        })
        // array: snapshots as mpenv_curriculum.SNAPSHOT records or uint8 [n, 176]
        .def("curriculum_pool_set", [](PySimManager &s, py::array array, int32_t map_range, int32_t first_slot) {
            py::array a = py::array::ensure(array, py::array::c_style);
            if (!a || a.nbytes() == 0 || a.nbytes() % (py::ssize_t)sizeof(mpenv_curriculum_snapshot) != 0)
                throw py::value_error("curriculum_pool_set: array must hold whole 176-byte snapshots, C-contiguous");
            check(mpenv_curriculum_pool_set(s.h->mgr, map_range, first_slot,
                                            (int32_t)(a.nbytes() / (py::ssize_t)sizeof(mpenv_curriculum_snapshot)),
                                            static_cast<const mpenv_curriculum_snapshot *>(a.data())));
        }, py::arg("array"), py::arg("map_range") = 0, py::arg("first_slot") = 0)
        .def("set_lidar_branch", [](PySimManager &s, bool on) { check(mpenv_set_lidar_branch(s.h->mgr, on ? 1 : 0)); })
        .def("set_lidar_iters", [](PySimManager &s, int32_t n) { check(mpenv_set_lidar_iters(s.h->mgr, n)); })
        .def("graph_status", [](PySimManager &s) {
            int32_t on = 0;
            char why[512] = {};
            check(mpenv_graph_status(s.h->mgr, &on, why, sizeof(why)));
            return py::make_tuple(on != 0, std::string(why));
        })
        .def("world_groups", [](PySimManager &s) { int32_t g = 0; check(mpenv_world_groups(s.h->mgr, &g)); return g; })
        .def("enable_kernel_timing", [](PySimManager &s, bool on) { check(mpenv_enable_kernel_timing(s.h->mgr, on)); })
        .def("enable_stats", [](PySimManager &s, bool on) { check(mpenv_enable_stats(s.h->mgr, on)); })
        .def("read_stats", [](PySimManager &s) {
            uint64_t v[10] = {};
            int n = mpenv_read_stats(s.h->mgr, v, 10);
            if (n < 0) check(n);
            static const char *names[10] = { "alive_agents", "los_pairs", "los_rays", "los_seen",
                                             "sphere_casts", "shot_rays", "hit_agents", "kills", "lk_rows",
                                             "los_traced" };
            py::dict d;
            for (int k = 0; k < 10; k++) d[py::str(names[k])] = v[k];
            return d;
        })
        .def("kernel_timings", [](PySimManager &s) {
            const char *names[16];
            float ms[16];
            int32_t launches[16];
            int n = mpenv_kernel_timings(s.h->mgr, 16, names, ms, launches);
            if (n < 0) check(n);
            py::dict d;
            for (int k = 0; k < n; k++) d[py::str(names[k])] = py::make_tuple(ms[k], launches[k]);
            return d;
        })
        .def_property_readonly("num_worlds", [](PySimManager &s) { int32_t w, n; mpenv_dims(s.h->mgr, &w, &n); return w; })
        .def_property_readonly("agents_per_world", [](PySimManager &s) { int32_t w, n; mpenv_dims(s.h->mgr, &w, &n); return n; })
        .def("fwd_lidar", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_FWD_LIDAR); })
        .def("rear_lidar", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_REAR_LIDAR); })
        .def("hp", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_HP); })
        .def("magazine", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_MAGAZINE); })
        .def("alive", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_ALIVE); })
        .def("self_obs", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_SELF_OBSERVATION); })
        .def("filters_state", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_FILTERS_STATE); })
        .def("teammates", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_TEAMMATE_OBSERVATIONS); })
        .def("opponents", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_OPPONENT_OBSERVATIONS); })
        .def("opponents_last_known",
             [](PySimManager &s) { return s.tensor(MPENV_EXPORT_OPPONENT_LAST_KNOWN_OBSERVATIONS); })
        .def("self_pos", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_SELF_POSITION); })
        .def("teammate_positions", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_TEAMMATE_POSITIONS); })
        .def("opponent_positions", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_OPPONENT_POSITIONS); })
        .def("opponent_last_known_positions",
             [](PySimManager &s) { return s.tensor(MPENV_EXPORT_OPPONENT_LAST_KNOWN_POSITIONS); })
        .def("opponent_masks", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_OPPONENT_MASKS); })
        .def("agent_map", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_AGENT_MAP); })
        .def("unmasked_agent_map", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_AGENT_MAP); })
        .def("reward_coefs", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_REWARD_HYPER_PARAMS); })
        .def("explore_action_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_EXPLORE_ACTION); })
        .def("pvp_action_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_PVP_DISCRETE_ACTION); })
        .def("aim_action_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_PVP_DISCRETE_AIM_ACTION); })
        .def("reward_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_REWARD); })
        .def("done_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_DONE); })
        .def("reset_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_RESET); })
        .def("self_observation_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_SELF_OBSERVATION); })
        // Extensions beyond bindings.cpp (Manager methods of mgr.hpp):
        .def("sim_control_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_SIM_CONTROL); })
        .def("match_result_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_MATCH_RESULT); })
        .def("policy_assignment_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_AGENT_POLICY); })
        .def("world_curriculum_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_WORLD_CURRICULUM); })
        .def("pvp_aim_action_tensor", [](PySimManager &s) { return s.tensor(MPENV_EXPORT_PVP_AIM_ACTION); })
        .def("export_tensor", [](PySimManager &s, int32_t id) { return s.tensor(id); })
        .def("trigger_reset", [](PySimManager &s, int32_t w) { check(mpenv_trigger_reset(s.h->mgr, w)); })
        .def("set_hp", [](PySimManager &s, int32_t w, int32_t a, int32_t hp) { check(mpenv_set_hp(s.h->mgr, w, a, hp)); })
        .def("set_agent_policy",
             [](PySimManager &s, int32_t w, int32_t a, int32_t p) { check(mpenv_set_agent_policy(s.h->mgr, w, a, p)); })
        .def("set_uniform_agent_policy",
             [](PySimManager &s, int32_t p) { check(mpenv_set_uniform_agent_policy(s.h->mgr, p)); })
        .def("train_interface", [](PySimManager &s) {
            int32_t ni = 0, no = 0;
            mpenv_train_interface_size(&ni, &no);
            py::dict inputs, outputs;
            for (int k = 0; k < ni; k++) {
                const char *name; int32_t id;
                mpenv_train_interface_entry(0, k, &name, &id);
                inputs[py::str(name)] = py::cast(s.tensor(id));
            }
            for (int k = 0; k < no; k++) {
                const char *name; int32_t id;
                mpenv_train_interface_entry(1, k, &name, &id);
                outputs[py::str(name)] = py::cast(s.tensor(id));
            }
            py::dict ti;
            ti["inputs"] = inputs;
            ti["outputs"] = outputs;
            return ti;
        })
        // JAXInterface::buildEntry (bindings.cpp:149-158): the XLA GPU
        // custom-call targets over gpuStreamInit / gpuStreamStep as PyCapsules
        // named "xla._CUSTOM_CALL_TARGET" (what jax's
        // xla_client.register_custom_call_target takes), the opaque bytes that
        // name this manager, and the trainInterface the call's operand
        // (inputs) and result (outputs) shapes come from.  Registering them
        // needs jax, absent from this image; the targets themselves are plain
        // C functions of XLA's API-version-1 signature, plus status-returning
        // twins (include/mpenv.h).
        .def("jax", [](PySimManager &s, bool xla_gpu) -> py::object {
            if (!xla_gpu)
                throw std::runtime_error("madrona_mp_env.SimManager.jax: only the XLA GPU (ROCm) target is built; "
                                         "ExecMode.CPU is not supported by this engine");
            mpenv_xla_opaque o;
            check(mpenv_xla_opaque_make(s.h->mgr, &o));
            const char *kName = "xla._CUSTOM_CALL_TARGET";
            py::dict d;
            d["init"] = py::capsule(reinterpret_cast<void *>(&mpenv_xla_gpu_stream_init), kName);
            d["step"] = py::capsule(reinterpret_cast<void *>(&mpenv_xla_gpu_stream_step), kName);
            d["opaque"] = py::bytes(reinterpret_cast<const char *>(&o), sizeof(o));
            // the same targets in XLA's status-returning form (API version 2,
            // API_VERSION_STATUS_RETURNING): failures reach XLA instead of
            // aborting the process
            d["init_status"] = py::capsule(reinterpret_cast<void *>(&mpenv_xla_gpu_stream_init_status), kName);
            d["step_status"] = py::capsule(reinterpret_cast<void *>(&mpenv_xla_gpu_stream_step_status), kName);
            d["platform"] = "ROCM";
            d["api_version"] = 1;
            d["status_api_version"] = 2;
            int32_t ni = 0, no = 0;
            mpenv_train_interface_size(&ni, &no);
            py::list in_names, out_names;
            for (int k = 0; k < ni; k++) {
                const char *name; int32_t id;
                mpenv_train_interface_entry(0, k, &name, &id);
                in_names.append(py::str(name));
            }
            for (int k = 0; k < no; k++) {
                const char *name; int32_t id;
                mpenv_train_interface_entry(1, k, &name, &id);
                out_names.append(py::str(name));
            }
            d["input_names"] = in_names;
            d["output_names"] = out_names;
            // keeps the manager alive as long as the registration data is
            d["sim"] = py::cast(s);
            return d;
        }, py::arg("xla_gpu") = true);

    // mpenv_state_section (no manager, no GPU): (name, offset, bytes,
    // row_bytes, row_kind, export_id, dtype, dims); dims are the export's for
    // an exported section, else (rows, elements per row).  idx -1: the blob.
    // mpenv_policy_check: validates a converted-checkpoint directory (no manager, no GPU)
    // what a scene directory asks of the engine (mpenv_scene_residency.h); no GPU, no manager
    m.def("scene_info", [](const std::string &path) {
        mpenv_scene_info_t i;
        check(mpenv_scene_info(path.c_str(), &i));
        py::dict d;
        d["triangles"] = i.triangles;
        d["collision_nodes"] = i.collision_nodes;
        d["collision_stack"] = i.collision_stack;
        d["lidar_nodes"] = i.lidar_nodes;
        d["lidar_stack"] = i.lidar_stack;
        d["lidar_triangles"] = i.lidar_triangles;
        d["lds_bytes"] = py::dict(py::arg("k_move") = i.lds_bytes_move, py::arg("k_sim") = i.lds_bytes_sim,
                                  py::arg("k_vis") = i.lds_bytes_vis, py::arg("k_lidar") = i.lds_bytes_lidar);
        d["global_bytes"] = i.global_bytes;
        d["residency"] = !i.supported ? py::object(py::none())
                                      : py::object(py::str(i.residency == MPENV_SCENE_LDS ? "lds" : "global"));
        d["supported"] = i.supported != 0;
        d["reason"] = std::string(i.reason);
        return d;
    }, py::arg("path"));
    // the camera model without a GPU (mpenv_camera.h): the two buffers' bytes for a batch, and the rays
    // of n agents -- pos [n, 3], aim_quat [n, 4] (w, x, y, z), cur_pose [n] -> (origins [n, 3],
    // directions [n, height, width, 3]), bit for bit what the kernel traces
    m.def("camera_layout", [](int32_t width, int32_t height, float hfov_deg, uint32_t num_worlds, uint32_t team_size) {
        const mpenv_camera_config c { width, height, hfov_deg, 0 };
        int64_t depth = 0, label = 0;
        check(mpenv_camera_layout(&c, num_worlds, team_size, &depth, &label));
        return py::dict(py::arg("shape") = py::make_tuple((int64_t)num_worlds * 2 * team_size, height, width),
                        py::arg("depth_bytes") = depth, py::arg("label_bytes") = label);
    }, py::arg("width"), py::arg("height"), py::arg("hfov_deg") = 90.0f, py::arg("num_worlds") = 1,
          py::arg("team_size") = 1);
    m.def("camera_rays", [](int32_t width, int32_t height, float hfov_deg,
                            py::array_t<float, py::array::c_style | py::array::forcecast> pos,
                            py::array_t<float, py::array::c_style | py::array::forcecast> aim_quat,
                            py::array_t<int32_t, py::array::c_style | py::array::forcecast> cur_pose) {
        const mpenv_camera_config c { width, height, hfov_deg, 0 };
        const py::ssize_t n = cur_pose.size();
        if (pos.size() != 3 * n || aim_quat.size() != 4 * n)
            throw py::value_error("camera_rays: pos must be [n, 3] and aim_quat [n, 4] for cur_pose [n]");
        int64_t unused = 0;
        check(mpenv_camera_layout(&c, 1, 1, &unused, nullptr)); // the configuration, before the outputs are sized by it
        py::array_t<float> org({ n, (py::ssize_t)3 });
        py::array_t<float> dir({ n, (py::ssize_t)height, (py::ssize_t)width, (py::ssize_t)3 });
        check(mpenv_camera_rays(&c, (int32_t)n, pos.data(), aim_quat.data(), cur_pose.data(), org.mutable_data(),
                                dir.mutable_data()));
        return py::make_tuple(org, dir);
    }, py::arg("width"), py::arg("height"), py::arg("hfov_deg"), py::arg("pos"), py::arg("aim_quat"),
          py::arg("cur_pose"));
    // what SimManager(scene_path=maps) would make of the list (mpenv_maps_plan): no GPU, no manager.  A
    // list the engine refuses raises with its message.
    m.def("maps_plan", [](py::object maps, uint32_t team_size, uint32_t sim_flags, Task task_type) {
        std::vector<std::string> paths;
        const std::vector<mpenv_map_range> ranges = mapRanges(maps, paths);
        mpenv_config cfg = {};
        cfg.exec_mode = MPENV_EXEC_CUDA;
        cfg.team_size = team_size;
        cfg.sim_flags = sim_flags;
        cfg.task_type = (int32_t)task_type;
        for (const mpenv_map_range &r : ranges) cfg.num_worlds += r.num_worlds;
        std::vector<mpenv_map_desc> desc(std::max<size_t>(ranges.size(), 1));
        int32_t track = 0;
        check(mpenv_maps_plan(&cfg, ranges.data(), (int32_t)ranges.size(), desc.data(), &track));
        py::list out;
        for (size_t r = 0; r < ranges.size(); r++)
            out.append(py::dict(py::arg("path") = paths[r], py::arg("first_world") = desc[r].first_world,
                                py::arg("num_worlds") = desc[r].num_worlds, py::arg("scene") = desc[r].scene,
                                py::arg("residency") = residencyName(desc[r].residency)));
        return py::dict(py::arg("maps") = out, py::arg("spawn_track_len") = track);
    }, py::arg("maps"), py::arg("team_size"), py::arg("sim_flags") = 0, py::arg("task_type") = Task::Zone);
    // the league's arithmetic without a GPU (mpenv_league.h): league_draw performs visit n of global
    // world `world` on ids [2, team_size] (weights [P+1, P], None: all 1) and returns the new ids;
    // league_record adds one ended episode (match_result: its first five values) to table
    // [P+1, P+1, 8] int64 in place and returns it
    m.def("league_draw", [](int32_t num_policies, const std::string &draw, uint32_t seed, uint32_t world, uint32_t n,
                            py::array_t<int32_t, py::array::c_style | py::array::forcecast> ids, py::object weights) {
        const mpenv_league_config c { num_policies, leagueDrawOf(draw), seed, 0 };
        int64_t unused = 0;
        check(mpenv_league_layout(&c, 1, &unused, nullptr, nullptr)); // the configuration, before sizes are checked by it
        if (ids.ndim() != 2 || ids.shape(0) != 2) throw py::value_error("league_draw: ids must be [2, team_size]");
        py::array_t<int32_t> out({ ids.shape(0), ids.shape(1) });
        std::copy(ids.data(), ids.data() + ids.size(), out.mutable_data());
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> w;
        if (!weights.is_none()) {
            w = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(weights);
            if (!w || w.size() != (py::ssize_t)(num_policies + 1) * num_policies)
                throw py::value_error("league_draw: weights must be [num_policies + 1, num_policies]");
        }
        check(mpenv_league_draw(&c, world, n, weights.is_none() ? nullptr : w.data(), (int32_t)ids.shape(1),
                                out.mutable_data()));
        return out;
    }, py::arg("num_policies"), py::arg("draw"), py::arg("seed"), py::arg("world"), py::arg("n"), py::arg("ids"),
          py::arg("weights") = py::none());
    m.def("league_record", [](int32_t num_policies, py::array_t<int32_t, py::array::c_style | py::array::forcecast> match_result,
                              py::array_t<int32_t, py::array::c_style | py::array::forcecast> ids,
                              py::array_t<int64_t, py::array::c_style> table) {
        const mpenv_league_config c { num_policies, MPENV_LEAGUE_DRAW_NONE, 0, 0 };
        int64_t bytes = 0;
        check(mpenv_league_layout(&c, 1, &bytes, nullptr, nullptr));
        if (match_result.size() < 5) throw py::value_error("league_record: match_result needs five values");
        if (ids.ndim() != 2 || ids.shape(0) != 2) throw py::value_error("league_record: ids must be [2, team_size]");
        if (table.nbytes() != bytes) throw py::value_error("league_record: table must be int64 [P + 1, P + 1, 8]");
        check(mpenv_league_record(&c, match_result.data(), ids.data(), (int32_t)ids.shape(1), table.mutable_data()));
        return table;
    }, py::arg("num_policies"), py::arg("match_result"), py::arg("ids"), py::arg("table"));
    // the curriculum pool's arithmetic without a GPU (mpenv_curriculum.h): curriculum_pool_select says
    // whether slot `slot` of range `range` refreshes at `tick` and names its candidate world;
    // curriculum_pool_pack packs one world (n = 2 * team_size agents) into its 176 bytes
    m.def("curriculum_pool_select", [](uint32_t seed, uint32_t world_id_offset, uint32_t range, uint32_t slot,
                                       uint32_t tick, int32_t period, int32_t first_world, int32_t num_worlds) {
        int32_t refresh = 0, world = -1;
        check(mpenv_curriculum_pool_select(seed, world_id_offset, range, slot, tick, period, first_world, num_worlds,
                                           &refresh, &world));
        return py::make_tuple(refresh != 0, world);
    }, py::arg("seed"), py::arg("world_id_offset"), py::arg("range"), py::arg("slot"), py::arg("tick"), py::arg("period"),
          py::arg("first_world"), py::arg("num_worlds"));
    m.def("curriculum_pool_pack", [](int32_t cur_step, int32_t cur_zone, int32_t captured, int32_t controlling,
                                     int32_t zone_steps, int32_t steps_until_point,
                                     py::array_t<float, py::array::c_style | py::array::forcecast> pos,
                                     py::array_t<float, py::array::c_style | py::array::forcecast> yaw,
                                     py::array_t<float, py::array::c_style | py::array::forcecast> pitch,
                                     py::array_t<float, py::array::c_style | py::array::forcecast> hp,
                                     py::array_t<int32_t, py::array::c_style | py::array::forcecast> magazine,
                                     py::array_t<int32_t, py::array::c_style | py::array::forcecast> cur_pose,
                                     py::array_t<int32_t, py::array::c_style | py::array::forcecast> landed_on) {
        const py::ssize_t n = yaw.size();
        if (n < 2 || n > 12 || n % 2 != 0) throw py::value_error("curriculum_pool_pack: 2 * team_size agents, team_size in [1, 6]");
        if (pos.size() != 3 * n || pitch.size() != n || hp.size() != n || magazine.size() != 2 * n || cur_pose.size() != n ||
            landed_on.size() != n)
            throw py::value_error("curriculum_pool_pack: pos [n, 3], magazine [n, 2], the rest [n]");
        const mpenv_curriculum_world w { cur_step, cur_zone, captured, controlling, zone_steps, steps_until_point,
                                         pos.data(), yaw.data(), pitch.data(), hp.data(), magazine.data(), cur_pose.data(),
                                         landed_on.data() };
        py::array_t<uint8_t> out((py::ssize_t)sizeof(mpenv_curriculum_snapshot));
        check(mpenv_curriculum_pool_pack(&w, (int32_t)(n / 2), reinterpret_cast<mpenv_curriculum_snapshot *>(out.mutable_data())));
        return out;
    }, py::arg("cur_step"), py::arg("cur_zone"), py::arg("captured"), py::arg("controlling"), py::arg("zone_steps"),
          py::arg("steps_until_point"), py::arg("pos"), py::arg("yaw"), py::arg("pitch"), py::arg("hp"), py::arg("magazine"),
          py::arg("cur_pose"), py::arg("landed_on"));
    m.attr("CURRICULUM_NEED_CAPTURED") = MPENV_CURRICULUM_NEED_CAPTURED;
    m.attr("CURRICULUM_NEED_CONTESTED") = MPENV_CURRICULUM_NEED_CONTESTED;
    m.attr("CURRICULUM_NEED_BOTH_ALIVE") = MPENV_CURRICULUM_NEED_BOTH_ALIVE;
    m.def("policy_check", [](const std::string &dir) { check(mpenv_policy_check(dir.c_str())); }, py::arg("dir"));
    m.def("state_section", [](int32_t idx, uint32_t num_worlds, uint32_t team_size, uint32_t spawn_track_len) {
        const char *name = nullptr;
        int64_t off = 0, bytes = 0;
        int32_t rb = 0, kind = 0, eid = -1, dt = MPENV_DTYPE_UINT8;
        check(mpenv_state_section(idx, num_worlds, team_size, spawn_track_len, &name, &off, &bytes, &rb, &kind, &eid));
        std::vector<int64_t> dims;
        if (idx >= 0) check(mpenv_state_section_dtype(idx, &dt));
        if (eid >= 0) {
            int32_t edt = 0, nd = 0;
            int64_t d[8];
            check(mpenv_export_layout(eid, num_worlds, team_size, &edt, &nd, d));
            dims.assign(d, d + nd);
        } else {
            const int64_t es = dt == MPENV_DTYPE_UINT8 ? 1 : dt == MPENV_DTYPE_UINT16 ? 2 : dt == MPENV_DTYPE_UINT64 ? 8 : 4;
            const int64_t rows = idx >= 0 ? bytes / rb : 1, per = idx >= 0 ? rb / es : bytes;
            dims = { rows, per };
        }
        static const char *const kNames[] = { "int32", "float32", "uint32", "uint8", "uint16", "uint64" };
        return py::make_tuple(std::string(name), off, bytes, rb, kind, eid, std::string(kNames[dt]),
                              py::tuple(py::cast(dims)));
    }, py::arg("idx"), py::arg("num_worlds"), py::arg("team_size"), py::arg("spawn_track_len") = 128);
}
