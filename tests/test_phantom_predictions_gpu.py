"""The phantom prediction kernels (fo_spawn_rule_predict_kernel, fo_spawn_predict_kernel: spawn_write_slot, heading_to_curve,
rl_lanelet_of_wave; csrc/fo_scene.hip, csrc/fo_spawn_rules.hpp) against the exact reference of tests/ref_phantom_predictions.py,
on the cases of tests/phantom_prediction_cases.py: every form the three scenario fixtures never select -- the second pass of the
closest-segment search and the fetch from the winner's lane, routes read from global memory (more than 256 vertices), horizons over
64 samples, more than 64 lanelets, ties, routes that end inside the horizon.  The maps go straight through the C ABI
(fo_scene_set_map / _set_centerlines / _set_routes), the point records are written into device memory by the test.
tests/test_phantom_predictions_cpu.py shows on the CPU that the cases select what they are meant to.  Needs a real MI355X."""
import ctypes as C_

import numpy as np
import pytest

import phantom_prediction_cases as C
import ref_phantom_predictions as R

pytestmark = pytest.mark.gpu

LAUNCHES = C.launches()
FILL = 7.25                      # what the output buffers hold before a call: the kernels write every row, zeros included


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


@pytest.fixture(scope="module")
def contexts(torch_cuda):
    """one context per map: polygons, centre lines, route table and lanelet raster through the C ABI"""
    from frenetix_occlusion import _native as N
    out = {}
    for name, make in C.SCENES.items():
        sc = make()
        ctx = N.Context(0)
        x0, y0, cs, nx, ny = C.RASTERS[name]
        off = np.zeros(len(sc.polys) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(p) for p in sc.polys])
        pxy = np.ascontiguousarray(np.concatenate(sc.polys), dtype=np.float64)
        org, dims = np.array([x0, y0], dtype=np.float64), np.array([nx, ny], dtype=np.int32)
        ctx.call("fo_scene_set_map", len(sc.polys), off.ctypes.data, pxy.ctypes.data, 0, None, cs, 2.0 * cs, None, org.ctypes.data,
                 dims.ctypes.data)
        coff, cxy = np.ascontiguousarray(sc.center_off, np.int32), np.ascontiguousarray(sc.center_xy, np.float64)
        ctx.call("fo_scene_set_centerlines", len(sc.polys), coff.ctypes.data, cxy.ctypes.data)
        ras = np.ascontiguousarray(C.lanelet_raster(name), dtype=np.int32)
        first, count = np.ascontiguousarray(sc.first, np.int32), np.ascontiguousarray(sc.count, np.int32)
        rxy, rs = np.ascontiguousarray(sc.xy, np.float64), np.ascontiguousarray(sc.s, np.float64)
        ctx.call("fo_scene_set_routes", len(sc.polys), 3, first.ctypes.data, count.ctypes.data, len(rs), rxy.ctypes.data, rs.ctypes.data,
                 ras.ctypes.data)
        out[name] = (ctx, ras)
    return out


def _buffers(torch, A, S, T):
    f = lambda *shape: torch.full(shape, FILL, dtype=torch.float64, device="cuda")
    i = lambda n: torch.full((n,), 77, dtype=torch.int32, device="cuda")
    return dict(pos0=f(A, 2), yaw0=f(A), pos=f(S, T, 2), yaw=f(S, T), v=f(S, T), cov=f(S, T, 4), shape=f(S, 2), raw=f(S, 2), type=i(S), len=i(S))


def _host(torch, b):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in b.items()}


def _check_static(launch_name, ref, got, n_slots):
    """type, inflated and raw dimensions of every slot, the inactive ones included"""
    assert np.array_equal(got["type"][:n_slots], ref["type"][:n_slots]), launch_name
    assert np.array_equal(got["shape"][:n_slots], ref["shape"][:n_slots]) and np.array_equal(got["raw"][:n_slots], ref["raw"][:n_slots])
    assert np.array_equal(got["cov"][:n_slots, :, 1:3], np.zeros_like(got["cov"][:n_slots, :, 1:3]))


WORST = {}


@pytest.mark.parametrize("launch", LAUNCHES, ids=[l.name for l in LAUNCHES])
def test_rule_agents_against_the_reference(torch_cuda, contexts, launch):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    ctx, _ = contexts[launch.map]
    ref = C.reference(launch)
    A, T = len(launch.points), launch.T
    S = 3 * A
    b = _buffers(torch, A, S, T)
    pts = torch.as_tensor(launch.points).cuda()
    npts = torch.tensor([launch.n_points], dtype=torch.int32, device="cuda")
    path = torch.as_tensor(launch.path).cuda()
    ty = N.RuleAgentTypes(*[(C_.c_double * 3)(*launch.types[k]) for k in ("speed", "raw_l", "raw_w", "infl_l", "infl_w")])
    ctx.call("fo_scene_spawn_rule_agents", A, pts.data_ptr(), npts.data_ptr(), 3, C_.byref(ty), len(launch.path), path.data_ptr(), T,
             launch.dt, C.VAR0, C.FACTOR, b["pos0"].data_ptr(), b["yaw0"].data_ptr(), b["pos"].data_ptr(), b["yaw"].data_ptr(),
             b["v"].data_ptr(), b["cov"].data_ptr(), b["shape"].data_ptr(), b["raw"].data_ptr(), b["type"].data_ptr(), b["len"].data_ptr(),
             N.current_stream(0))
    got = _host(torch, b)
    n = launch.n_points
    w = C.compare(launch, ref, got, "device", range(S), WORST)            # live and inactive slots: len, values, zeros behind len
    print(launch.name, {k: f"{v:.3g}" for k, v in w.items()})
    _check_static(launch.name, ref, got, S)
    assert np.array_equal(got["pos0"], ref["pos0"]), launch.name           # (zeros for the points that do not exist)
    dev = np.abs(got["yaw0"] - ref["yaw0"])
    assert dev.max() <= 1e-12, (launch.name, launch.tags[int(dev[:n].argmax())] if dev[:n].max() > 1e-12 else "inactive", dev.max())
    assert np.all(got["len"][3 * n:] == 0) and np.all(got["yaw0"][n:] == 0.0)


@pytest.mark.parametrize("T", [31, 65])
@pytest.mark.parametrize("name", ["LONG", "MANY"])
def test_cell_sampler_against_the_reference(torch_cuda, contexts, name, T):
    """fo_scene_spawn on a hand-written class array (a handful of occluded cells, all_occluded, three routes): the reference at the
    cell centres the call reports, the lanelet from the lanelet raster there"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    ctx, ras = contexts[name]
    x0, y0, cs, nx, ny = C.RASTERS[name]
    cells = C.occluded_cells(name)
    cls = np.ones((ny, nx), dtype=np.uint8)
    for ix, iy in cells:
        cls[iy, ix] = 5                                            # road + occluded
    A = len(cells) + 3
    S = 3 * A
    b = _buffers(torch, A, S, T)
    cell = torch.full((A,), 77, dtype=torch.int32, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_cls = torch.as_tensor(cls).cuda()
    path_np = C.long_paths()[129] if name == "LONG" else C.MANY_PATH
    path = torch.as_tensor(np.ascontiguousarray(path_np)).cuda()
    t = C.TYPES
    idx = [{C.CAR: 0, C.BIKE: 1, C.PED: 2}[p] for p in C.PATTERN]
    t4 = np.array(C.PATTERN, dtype=np.int32)
    arr = {k: np.array([t[k][i] for i in idx], dtype=np.float64) for k in ("speed", "raw_l", "raw_w", "infl_l", "infl_w")}
    c = lambda a: a.ctypes.data
    ctx.call("fo_scene_spawn", d_cls.data_ptr(), 0, 0, nx, ny, 0.0, 0.0, 1.0, 0.0, -1.0e9, 1.0e9, 1, A, 3, c(t4), c(arr["speed"]),
             c(arr["raw_l"]), c(arr["raw_w"]), c(arr["infl_l"]), c(arr["infl_w"]), len(path_np), path.data_ptr(), T, 0.1, C.VAR0, C.FACTOR,
             cell.data_ptr(), b["pos0"].data_ptr(), b["yaw0"].data_ptr(), n_out.data_ptr(), b["pos"].data_ptr(), b["yaw"].data_ptr(),
             b["v"].data_ptr(), b["cov"].data_ptr(), b["shape"].data_ptr(), b["raw"].data_ptr(), b["type"].data_ptr(), b["len"].data_ptr(),
             N.current_stream(0))
    got = _host(torch, b)
    n = int(n_out.item())
    assert n == len(cells)
    assert cell.cpu().numpy().tolist() == [iy * nx + ix for ix, iy in cells] + [-1] * 3
    centres = np.array([(x0 + (ix + 0.5) * cs, y0 + (iy + 0.5) * cs) for ix, iy in cells])
    assert np.array_equal(got["pos0"][:n], centres) and np.all(got["pos0"][n:] == 0.0)
    recs = np.array([C.rec(C.PATTERN[j % 4], *(got["pos0"][j] if j < n else (0.0, 0.0))) for j in range(A)])
    lan = [int(ras[iy, ix]) for ix, iy in cells]
    scene = C.SCENES[name]()
    ref = R.predict(scene, recs, n, path_np, T, 0.1, C.VAR0, C.FACTOR, t["speed"], t["raw_l"], t["raw_w"], t["infl_l"], t["infl_w"],
                    entry="cells", lanelets=lan)
    for j, (ix, iy) in enumerate(cells):                           # the raster's lanelet is the first one that holds the centre
        assert R.lanelet_of(scene, R.Fr(float(centres[j, 0])), R.Fr(float(centres[j, 1])))[0] == lan[j]
    assert not [s for s in range(3 * n) if ref["status"][s] == "open"]
    launch = C.Launch(f"cells {name} T={T}", name, recs, n, [f"cell {c_}" for c_ in cells], path_np, T, 0.1)
    w = C.compare(launch, ref, got, "cell sampler", range(S), WORST)
    print(launch.name, {k: f"{v:.3g}" for k, v in w.items()})
    _check_static(launch.name, ref, got, S)
    assert np.abs(got["yaw0"] - ref["yaw0"]).max() <= 1e-12
    routed = [s for s in range(3 * n) if ref["dec"][s] is not None and ref["dec"][s]["form"] == "route"]
    assert len(routed) >= 12 and any(0 < ref["len"][s] < T for s in routed)
    if name == "MANY":
        assert {3, 64, 70, 129} <= set(lan)
    else:
        assert any(ref["dec"][s]["nv"] > 256 for s in routed) and any(ref["dec"][s]["seg"] >= 64 for s in routed)
        empty = [j for j in range(n) if lan[j] == C.L_ONE and C.PATTERN[j % 4] != C.PED]
        assert empty and all(ref["len"][3 * j + r] == 0 for j in empty for r in range(3))   # [1, 0, 0]: routed, no route of two vertices
