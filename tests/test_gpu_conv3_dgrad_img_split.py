"""Split-mode image-resident conv3 data gradient (csrc/conv3_dgrad_img_split.hip) against the
generic implicit GEMM it replaces (igemm_dma_kernel<1, true, true, 9, 81, true, 2, 64>) and
against fp64.

The new kernel reproduces the generic kernel's arithmetic (the same MFMA shape and operand
roles, one accumulator chain per output over the same K order, the same three products per
sub-step, the same split and mask), so both output planes are the same bits; both kernels are
bounded against an fp64 conv_transpose2d with the tolerance tests/test_gpu_split.py applies to
this layer's data gradient (TOL, relative L2).
"""
import pytest
import torch

from apex_dqn_amd.ops.switches import SW

DEV = torch.device("cuda", 0)
TOL = 1e-4          # tests/test_gpu_split.py TOL (test_conv_split_dgrad)
# (images, grid; 0 = the launcher's default of 256 workgroups, capped to the images)
CASES = [
    (1, 0),
    (2, 0),
    (5, 2),      # workgroup 0 walks 3 images, workgroup 1 two: an uneven last round, and a
                 # prefetch of a next image that does not exist
    (3, 0),      # the default grid capped to N
    (257, 0),    # one workgroup with two images, the rest with one
]


def _lib():
    from apex_dqn_amd.ops import _lib as L
    return L.require_kernels()


def _split(x32):
    x32 = x32.to(DEV, torch.float32)
    hi = x32.to(torch.bfloat16)
    return hi, (x32 - hi.float()).to(torch.bfloat16)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _ref64(dy32, w32, y2):
    """fp64 conv_transpose2d of the fp32 operands times the ReLU mask of y2 (NHWC)."""
    dx = torch.nn.functional.conv_transpose2d(dy32.double().cpu().permute(0, 3, 1, 2),
                                              w32.double().cpu().permute(0, 3, 1, 2))      # OHWI -> OIHW
    return dx.permute(0, 2, 3, 1) * (y2.double().cpu() > 0)


def _make(N, seed, dy_fn=None, mask_fn=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w32 = torch.randn(64, 3, 3, 64, generator=g) * 0.04
    dy32 = torch.randn(N, 7, 7, 64, generator=g)
    y2 = torch.relu(torch.randn(N, 9, 9, 64, generator=g))      # about half the mask is zero
    if dy_fn is not None:
        dy32 = dy_fn(dy32)
    if mask_fn is not None:
        y2 = mask_fn(y2)
    y2 = y2.to(DEV, torch.bfloat16)
    dyh, dyl = _split(dy32)
    wh, wl = _split(w32)
    return dict(dyh=dyh, dyl=dyl, wh=wh, wl=wl, y2=y2, ref=_ref64(dy32, w32, y2))


_INPUTS = {}


def _inputs(N):
    """Operand planes and the fp64 reference of one batch size (computed once, never changed)."""
    if N not in _INPUTS:
        _INPUTS[N] = _make(N, N + 23)
    return _INPUTS[N]


def _nan_planes(N):
    return (torch.full((N, 9, 9, 64), float("nan"), dtype=torch.bfloat16, device=DEV),
            torch.full((N, 9, 9, 64), float("nan"), dtype=torch.bfloat16, device=DEV))


def _run_img(c, grid):
    from apex_dqn_amd.ops import conv as C
    hi, lo = _nan_planes(c["dyh"].shape[0])
    C.conv3_dgrad_img_split(_lib(), c["dyh"], c["dyl"], c["wh"], c["wl"], c["y2"], hi, lo, grid=grid)
    torch.cuda.synchronize()
    return hi, lo


def _run_generic(c, monkeypatch):
    from apex_dqn_amd.ops import conv as C
    monkeypatch.setattr(SW, "conv3_dgrad_img_split", False)
    hi, lo = _nan_planes(c["dyh"].shape[0])
    C.conv3_dgrad(_lib(), c["dyh"], c["wh"], c["y2"], hi, dy_lo=c["dyl"], w_lo=c["wl"], out_lo=lo)
    torch.cuda.synchronize()
    return hi, lo


def _bits(t):
    return t.view(torch.int16)


def _check(c, grid, monkeypatch, what):
    gh, gl = _run_generic(c, monkeypatch)
    ih, il = _run_img(c, grid)
    e = dict(img=_rel(ih.double() + il.double(), c["ref"]), generic=_rel(gh.double() + gl.double(), c["ref"]))
    print(f"{what}: relative error vs fp64:", {k: f"{v:.2e}" for k, v in e.items()})
    assert torch.equal(_bits(ih), _bits(gh))
    assert torch.equal(_bits(il), _bits(gl))
    assert max(e.values()) < TOL, e
    return ih, il


@pytest.mark.gpu
@pytest.mark.parametrize("N,grid", CASES)
def test_same_bits_as_generic_and_within_tol_of_fp64(N, grid, monkeypatch):
    _check(_inputs(N), grid, monkeypatch, f"N={N} grid={grid}")


@pytest.mark.gpu
def test_corner_pixels_only(monkeypatch):
    """dY3 non-zero only in its four corner pixels: every output pixel reads mostly the zero
    ring, and the outer output ring sees exactly one tap."""
    def corners(dy):
        out = torch.zeros_like(dy)
        for i in (0, 6):
            for j in (0, 6):
                out[:, i, j] = dy[:, i, j]
        return out
    c = _make(2, 101, dy_fn=corners)
    ih, il = _check(c, 0, monkeypatch, "corners")
    # output pixels out of every corner's 3 x 3 reach are exact zeros in both planes
    assert not _bits(ih[:, 3:6, :]).any() and not _bits(il[:, 3:6, :]).any()
    assert not _bits(ih[:, :, 3:6]).any() and not _bits(il[:, :, 3:6]).any()
    assert _bits(ih).any()


@pytest.mark.gpu
def test_all_zero_mask(monkeypatch):
    """y2 = 0 everywhere: both planes are zero bits, the lo plane's residuals included."""
    c = _make(2, 102, mask_fn=torch.zeros_like)
    ih, il = _check(c, 0, monkeypatch, "zero mask")
    assert not _bits(ih).any() and not _bits(il).any()


@pytest.mark.gpu
def test_launcher_refuses_uncovered_problems():
    """Wrong shapes, a missing plane and a misaligned pointer give an error and launch
    nothing: the NaN-filled outputs stay untouched."""
    from apex_dqn_amd.ops import _lib as L
    from apex_dqn_amd.ops.conv_sigs import Conv3DgradSplitDesc
    lib = _lib()
    c = _inputs(2)
    hi, lo = _nan_planes(2)

    def desc(**kw):
        a = dict(dy=c["dyh"].data_ptr(), dy_lo=c["dyl"].data_ptr(), w=c["wh"].data_ptr(), w_lo=c["wl"].data_ptr(),
                 mask=c["y2"].data_ptr(), dx=hi.data_ptr(), dx_lo=lo.data_ptr(), N=2, H=7, W=7, Cout=64, Cin=64,
                 KH=3, KW=3, stride=1)
        a.update(kw)
        d = Conv3DgradSplitDesc()
        for k, v in a.items():
            setattr(d, k, v)
        return d

    st = L.stream_ptr()
    run = lib.apex_conv3_dgrad_img_split
    bad = [dict(N=0), dict(H=9, W=9), dict(W=8), dict(Cout=32), dict(Cin=128), dict(KH=4, KW=4), dict(KW=1),
           dict(stride=2), dict(dy_lo=None), dict(w_lo=None), dict(dx_lo=None), dict(mask=None),
           dict(dy=c["dyh"].data_ptr() + 2), dict(dx_lo=lo.data_ptr() + 8), dict(w=c["wh"].data_ptr() + 4)]
    for kw in bad:
        assert run(desc(**kw), 0, st) != 0, kw
    assert run(desc(), -1, st) != 0
    torch.cuda.synchronize()
    assert torch.isnan(hi).all() and torch.isnan(lo).all()
    assert run(desc(), 0, st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(hi).any() and not torch.isnan(lo).any()


def _learner(B, monkeypatch):
    import numpy as np
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    monkeypatch.setattr(SW, "bwd_branches", True)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                "Learner": {"replay_sample_size": B},
                                "Runtime": {"use_graphs": False, "presample": False, "dtype": "fp32"}})
    torch.manual_seed(0)
    rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
    rng = np.random.default_rng(11)
    seqs = rp.append_frames(rng.integers(0, 255, (1800, 84, 84), dtype=np.uint8))
    K = 1500
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, 6, K), R=rng.normal(size=K) * 2,
                   Gamma=np.where(rng.random(K) < 0.1, 0.0, 0.97), priority=rng.random(K)))
    L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
    assert L.split and L._branched
    return L


@pytest.mark.gpu
def test_learner_three_updates_switch_on_vs_off(monkeypatch):
    """Three eager fp32 updates of a 24-row batch from the same seed, with the image-resident
    kernel (threshold 0) and with the generic one: parameters, optimizer state and TD errors
    (the priorities) are the same bits."""
    from apex_dqn_amd.ops import conv as C
    picks, res = [], {}
    real = C.conv3_dgrad_img_split_pick
    monkeypatch.setattr(C, "conv3_dgrad_img_split_pick",
                        lambda *a, **k: (picks.append(real(*a, **k)), picks[-1])[1])
    monkeypatch.setattr(SW, "conv3_dgrad_img_split_min", 0)
    for on in (True, False):
        monkeypatch.setattr(SW, "conv3_dgrad_img_split", on)
        del picks[:]
        L = _learner(24, monkeypatch)
        for _ in range(3):
            L.step()
        torch.cuda.synchronize()
        # conv3's data gradient asks once per update
        assert len(picks) == 3 and sum(picks) == (3 if on else 0)
        res[on] = {k: getattr(L, k).clone() for k in ("p32", "rms_v", "rms_m", "td_abs")}
    for k in res[True]:
        assert torch.equal(res[True][k], res[False][k]), k


def test_gating_picks_the_image_kernel_only_where_it_applies(monkeypatch):
    """CPU: the covered shape in split mode only, the switch on and the batch at or above the
    threshold; a forced choice overrides the switch and the threshold but not the coverage."""
    from apex_dqn_amd.ops import conv as C
    w = (64, 3, 3, 64)
    pick = C.conv3_dgrad_img_split_pick

    def shp(n, h=7, c=64, o=9):
        return (n, h, h, c), w, (n, o, o, c)

    monkeypatch.setattr(SW, "conv3_dgrad_img_split", True)
    monkeypatch.setattr(SW, "conv3_dgrad_img_split_min", 256)
    assert pick(*shp(512), True)
    assert pick(*shp(256), True)
    assert not pick(*shp(255), True)                                  # below the threshold
    assert not pick(*shp(512), False)                                 # bf16 learner
    assert not pick(*shp(512, h=9, o=11), True)
    assert not pick(*shp(512, c=32), True)
    assert not pick((512, 7, 7, 64), (64, 4, 4, 64), (512, 9, 9, 64), True)
    assert not pick((512, 7, 7, 64), w, (512, 10, 10, 64), True)
    assert not pick((512, 7, 7, 64), w, (511, 9, 9, 64), True)
    monkeypatch.setattr(SW, "conv3_dgrad_img_split_min", 0)
    assert pick(*shp(1), True)
    monkeypatch.setattr(SW, "conv3_dgrad_img_split", False)
    assert not pick(*shp(512), True)
    # forced (tests): overrides switch and threshold ...
    assert pick(*shp(1), True, force=True)
    monkeypatch.setattr(SW, "conv3_dgrad_img_split", True)
    assert not pick(*shp(512), True, force=False)
    # ... but not the coverage
    with pytest.raises(ValueError):
        pick(*shp(512), False, force=True)
