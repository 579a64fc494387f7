"""ctypes access to libmp_plan_probe.so: the launch plans of minipath_amd/csrc/launch_plan.cpp and the kernel table, host code only."""
import ctypes as C
import os

from tests import dispatch_cases as dc
from tests.conftest import ROOT

CUS = 256  # MI355X
LDS_CU = 160 * 1024
MP_ERR_UNSUPPORTED = 5
RENDER, AOV, STAGED, TRACE, BOUNDED, OCCLUDED = range(6)
API = {"render": RENDER, "paths": RENDER, "wf": STAGED, "aov": AOV, "trace": TRACE, "bounded": BOUNDED, "occluded": OCCLUDED}

_IN = ["kind", "inst_count", "inner_count", "packet_count", "stack_cap", "packet_stack_regs", "boxes_ordered", "tris_bounded", "materials_rgb",
       "n_tiles", "tile_size", "spp", "pass_begin", "pass_end", "cu_count", "traversal", "max_depth", "chunked",
       "packet_samples", "rays_per_lane", "mask_cache", "paths_pooled"]


class PlanIn(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in _IN]


class PlanOut(C.Structure):
    _fields_ = [("rc", C.c_int32), ("error", C.c_char * 128), ("kernel", C.c_int32), ("grid", C.c_uint32), ("lds", C.c_uint32),
                ("lds_per_wave", C.c_uint32), ("pool_stride", C.c_uint32), ("pool_bytes", C.c_uint64), ("units2", C.c_uint64),
                ("vertex", C.c_int32), ("trace", C.c_int32)] + [(n, C.c_uint32) for n in (
                    "trace_lds", "trace_lds_per_wave", "trace_grid", "sc", "tb", "n_max", "nbins", "nchan", "cam_grid", "flat_grid", "px_grid")] + [
                ("ws_bytes", C.c_uint64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        # MP_PLAN_PROBE_SO: the sanitizer build of the same probe (tools/asan_cpu_tests.sh)
        _lib = C.CDLL(os.environ.get("MP_PLAN_PROBE_SO") or os.path.join(ROOT, "minipath_amd", "csrc", "libmp_plan_probe.so"))
        _lib.mp_plan_kernel_name.restype = C.c_char_p
        _lib.mp_plan.argtypes = [C.c_int, C.POINTER(PlanIn), C.c_uint64, C.POINTER(PlanOut)]
        _lib.mp_plan.restype = None
    return _lib


def table():
    """the names of the kernel table, by id"""
    return [lib().mp_plan_kernel_name(i).decode() for i in range(lib().mp_plan_kernel_count())]


def launch(facts, n_tiles, tile_size, spp, passes=None, cus=CUS, traversal=0, max_depth=0, chunked=0, samples=0, lanes=1, cache=1, pooled=1, regs=64):
    """the fields of a RenderLaunch a plan reads; facts as dispatch_cases.scene_facts gives them"""
    begin, count = passes if passes else (0, spp)
    return PlanIn(kind=facts["kind"], inst_count=facts["members"], inner_count=facts["nodes"], packet_count=facts["packets"],
                  stack_cap=facts["stack_bound"], packet_stack_regs=regs, boxes_ordered=facts["boxes_ordered"], tris_bounded=facts["tris_bounded"],
                  materials_rgb=facts.get("rgb", 0), n_tiles=n_tiles, tile_size=tile_size, spp=spp, pass_begin=begin, pass_end=begin + count,
                  cu_count=cus, traversal=traversal, max_depth=max_depth, chunked=chunked, packet_samples=samples, rays_per_lane=lanes,
                  mask_cache=cache, paths_pooled=pooled)


def plan(api, inp, n_rays=0):
    out = PlanOut()
    lib().mp_plan(api, C.byref(inp), n_rays, C.byref(out))
    return out


def name(out, field="kernel"):
    return lib().mp_plan_kernel_name(getattr(out, field)).decode()


def row_input(row, passes=None, tiling=None):
    """a row of dispatch_cases as the GPU matrix runs it: its frame, its options; tiling = (tile_size, tile count) of another
    tile list over the same frame (tests/tile_geometries.py)"""
    o = {**dc.DEFAULTS, **row["opts"]}
    res, ts = (dc.AOV_RES, dc.AOV_TS) if row["api"] == "aov" else (dc.RES, dc.TS)
    n_tiles = -(-res[0] // ts) * -(-res[1] // ts)
    if tiling is not None:
        ts, n_tiles = tiling
    return launch(dc.scene_facts(row["scene"]), n_tiles, ts, row["spp"], passes, traversal=1 if row["traversal"] == "groups" else 0,
                  max_depth=dc.DEPTH if row["api"] in ("paths", "wf") else 0, samples=o["packet_samples_in_flight"], lanes=o["packet_rays_per_lane"],
                  cache=o["packet_mask_cache"], pooled=o["paths_pooled"], regs=o["packet_stack_registers"])


def row_names(row, passes=None, tiling=None):
    """every kernel name the plans give for the row's call"""
    api = API[row["api"]]
    out = plan(api, row_input(row, passes, tiling), dc.N_RAYS)
    assert out.rc == 0, out.error
    if api == STAGED:
        return {name(out), name(out, "vertex"), name(out, "trace"), "wf_scan_kernel", "wf_scatter_kernel", "wf_accumulate_kernel"}
    return {name(out)}
