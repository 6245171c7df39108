"""Image-resident conv3 weight gradient (csrc/conv3_wgrad_img.hip) against fp64 and against
the generic split-mode kernel it replaces at large batches (igemm_wgrad_kernel<1, 7, 49, 1,
3, 1>).

The oracle is the formula of ops/reference.py conv_wgrad evaluated in float64 on the hi + lo
planes reconstructed in float64.  The new kernel sums per-image chunks over a contiguous
image range per workgroup, the generic one 64-row steps over 384-row (192 below 256 images)
splits: the same three bf16 products per term with fp32 accumulation in another order, so
the bits differ.  Bound: normalised max error (max |got - ref| / max |ref|) at most twice
the generic kernel's on the same inputs, and under tests/test_gpu_split.py's TOL.
"""
import pytest
import torch

from apex_dqn_amd.ops.switches import SW

DEV = torch.device("cuda", 0)
TOL = 1e-4          # tests/test_gpu_split.py TOL
# (images, grids): 1 and 2 workgroups, uneven ranges, one image per workgroup, and more
# workgroups than images (the launcher's caller clamps the grid: no empty workgroup exists)
CASES = [(1, (1, 4)), (2, (1, 2, 5)), (3, (1, 2, 3)), (5, (1, 2, 3, 8)), (74, (1, 2, 7, 74, 128))]


def _lib():
    from apex_dqn_amd.ops import _lib as L
    return L.require_kernels()


def _split(x32):
    x32 = x32.to(DEV, torch.float32)
    hi = x32.to(torch.bfloat16)
    return hi, (x32 - hi.float()).to(torch.bfloat16)


def _nmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


_INPUTS = {}


def _inputs(N):
    """Operand planes (with a NaN guard image behind image N - 1), the fp64 reference and the
    generic kernel's result of one batch size: computed once, never changed."""
    if N in _INPUTS:
        return _INPUTS[N]
    g = torch.Generator(device="cpu").manual_seed(N + 33)
    dy32 = torch.randn(N, 7, 7, 64, generator=g)
    y32 = torch.relu(torch.randn(N, 9, 9, 64, generator=g))       # about half exact zeros
    y32[:, 4] = 0.0                                               # a whole zero row of every image
    y32[0, :, 0] = 0.0                                            # and a zero column of the first
    y32[N - 1, 8, 8] = 0.0
    nan = torch.full((1, 1, 1, 1), float("nan"))
    planes = {}
    for name, t in (("dy", dy32), ("y", y32)):
        hi, lo = _split(torch.cat([t, nan.expand(1, *t.shape[1:])]))
        assert torch.isnan(hi[N]).all() and torch.isnan(lo[N]).all()
        planes[name + "h"], planes[name + "l"] = hi[:N], lo[:N]   # contiguous views; image N is the guard
    dy64 = planes["dyh"].double().cpu() + planes["dyl"].double().cpu()
    y64 = planes["yh"].double().cpu() + planes["yl"].double().cpu()
    rdw = torch.nn.grad.conv2d_weight(y64.permute(0, 3, 1, 2), (64, 64, 3, 3), dy64.permute(0, 3, 1, 2),
                                      stride=1).permute(0, 2, 3, 1).contiguous()          # OIHW -> OHWI
    c = dict(planes, rdw=rdw, rdb=dy64.sum((0, 1, 2)), N=N)
    dw, db, _ = _run(c, None)
    c["gdw"], c["gdb"] = dw, db
    c["generic_err"] = (_nmax(dw, rdw), _nmax(db, c["rdb"]))
    _INPUTS[N] = c
    return c


def _run(c, grid):
    """dW3, db3 through the deferred job and grad_finalize; ``grid`` None: the generic kernel."""
    from apex_dqn_amd.ops import conv as C
    ws = C.Workspace()
    N = c["N"]
    if grid is not None:       # NaN-filled slabs of the size the op will ask for: an unwritten element shows
        G = min(grid, N)
        ws.get(("wg3img", G), G * 64 * 576, DEV).fill_(float("nan"))
        ws.get(("wg3imgb", G), G * 64, DEV).fill_(float("nan"))
    dw = torch.full((64, 3, 3, 64), float("nan"), device=DEV)
    db = torch.full((64,), float("nan"), device=DEV)
    jobs = []
    C.conv_wgrad(_lib(), ws, c["dyh"], c["yh"], 3, 1, dw, db, jobs=jobs, dy_lo=c["dyl"], x_lo=c["yl"],
                 img_kernel=grid is not None, img_grid=grid or 0)
    assert len(jobs) == 1
    C.finalize_grads(_lib(), jobs)
    torch.cuda.synchronize()
    return dw, db, jobs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("N,grids", CASES)
def test_within_twice_the_generic_error_of_fp64(N, grids):
    c = _inputs(N)
    ge_w, ge_b = c["generic_err"]
    print(f"N={N} generic kernel normalised max error vs fp64: dW {ge_w:.2e} db {ge_b:.2e}")
    assert ge_w < TOL and ge_b < TOL
    for grid in grids:
        dw, db, job = _run(c, grid)
        G = min(grid, N)
        assert job["nsplit"] == G and job["n"] == 64 * 576 and job["nb"] == 64
        # every element of the planes the finalize job reads was written (NaN-filled before)
        assert torch.isfinite(job["slab"][:G * 64 * 576]).all() and torch.isfinite(job["bslab"][:G * 64]).all()
        ew, eb = _nmax(dw, c["rdw"]), _nmax(db, c["rdb"])
        print(f"N={N} grid={grid} image-resident normalised max error vs fp64: dW {ew:.2e} db {eb:.2e}")
        assert torch.isfinite(dw).all() and torch.isfinite(db).all()     # the NaN guard image was not read
        assert ew <= 2 * ge_w and eb <= 2 * ge_b, (grid, ew, ge_w, eb, ge_b)
        assert ew < TOL and eb < TOL
        dw2, db2, _ = _run(c, grid)                                      # a fixed grid gives the same bits
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.gpu
def test_direct_reduce_path_matches_the_job_path():
    """Without ``jobs`` the launcher reduces the slab itself: the same bits as grad_finalize."""
    from apex_dqn_amd.ops import conv as C
    c = _inputs(5)
    dw, db, _ = _run(c, 3)
    dw2 = torch.full((64, 3, 3, 64), float("nan"), device=DEV)
    db2 = torch.full((64,), float("nan"), device=DEV)
    C.conv_wgrad(_lib(), C.Workspace(), c["dyh"], c["yh"], 3, 1, dw2, db2, dy_lo=c["dyl"], x_lo=c["yl"],
                 img_kernel=True, img_grid=3)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.gpu
def test_launcher_refuses_uncovered_problems():
    """The launcher runs only the split-mode conv3 shape without fused norm partials, with
    1 .. N workgroups."""
    from apex_dqn_amd.ops import _lib as L
    from apex_dqn_amd.ops import conv as C
    lib = _lib()
    c = _inputs(2)
    slab, bslab = torch.empty(2 * 64 * 576, device=DEV), torch.empty(2 * 64, device=DEV)
    part = torch.zeros(64, dtype=torch.float64, device=DEV)

    def desc(**kw):
        a = dict(dy=c["dyh"].data_ptr(), x=c["yh"].data_ptr(), slab=slab.data_ptr(), bias_slab=bslab.data_ptr(),
                 N=2, H=9, W=9, Cin=64, OH=7, OW=7, KH=3, KW=3, stride=1, mode=1, Co=64, Kc=576, ldd=64,
                 rows_per_split=0, Mred=98, dy_lo=c["dyl"].data_ptr(), x_lo=c["yl"].data_ptr())
        a.update(kw)
        return C._wg_desc(**a)

    st = L.stream_ptr()
    assert lib.apex_conv3_wgrad_img(desc(), None, None, 2, 1.0, st) == 0
    assert lib.apex_conv3_wgrad_img(desc(), None, None, 1, 1.0, st) == 0
    assert lib.apex_conv3_wgrad_img(desc(), None, None, 3, 1.0, st) != 0          # an empty workgroup
    assert lib.apex_conv3_wgrad_img(desc(), None, None, 0, 1.0, st) != 0
    assert lib.apex_conv3_wgrad_img(desc(x_lo=None), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv3_wgrad_img(desc(dy_lo=None), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv3_wgrad_img(desc(norm_part=part.data_ptr()), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv3_wgrad_img(desc(Mred=97), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv3_wgrad_img(desc(H=20, W=20, OH=9, OW=9, KH=4, KW=4, stride=2, Kc=1024), None, None, 1, 1.0,
                                    st) != 0
    torch.cuda.synchronize()


def test_gating_picks_the_image_kernel_only_where_it_applies(monkeypatch):
    """CPU: the covered shape and mode only, the switch on and the batch at or above the
    threshold; a forced choice overrides the switch and the threshold but not the coverage."""
    from apex_dqn_amd.ops import conv as C
    y2, dy3 = (512, 9, 9, 64), (512, 7, 7, 64)
    pick = C.conv3_wgrad_img_pick
    monkeypatch.setattr(SW, "conv3_wgrad_img", True)
    monkeypatch.setattr(SW, "conv3_wgrad_img_min", 256)
    assert pick(y2, dy3, 3, 1, True)
    assert pick((256, 9, 9, 64), (256, 7, 7, 64), 3, 1, True)
    assert not pick((255, 9, 9, 64), (255, 7, 7, 64), 3, 1, True)                 # below the threshold
    assert not pick(y2, dy3, 3, 1, False)                                         # bf16 learner
    assert not pick((512, 20, 20, 64), (512, 9, 9, 64), 4, 2, True)               # conv2
    assert not pick((512, 9, 9, 32), dy3, 3, 1, True)
    assert not pick(y2, (511, 7, 7, 64), 3, 1, True)
    assert not pick(y2, dy3, 3, 2, True)
    monkeypatch.setattr(SW, "conv3_wgrad_img", False)
    assert not pick(y2, dy3, 3, 1, True)
    assert pick((1, 9, 9, 64), (1, 7, 7, 64), 3, 1, True, force=True)             # forced: switch and threshold ...
    monkeypatch.setattr(SW, "conv3_wgrad_img", True)
    assert not pick(y2, dy3, 3, 1, True, force=False)
    with pytest.raises(ValueError):                                               # ... but not the coverage
        pick(y2, dy3, 3, 1, False, force=True)
