"""conv2 data gradient fused with conv1 weight gradient (csrc/conv21_bwd_fused.hip) against
the pair of kernels it replaces at large batches -- conv2_dgrad_img_split_kernel +
conv1_wgrad_img_kernel<4, true> -- and against fp64.

dY1 (debug store) is bit-identical to the per-image dgrad kernel's planes; dW1 / db1 are
bounded against fp64 with the replaced kernel's own tolerance (tests/test_gpu_split.py TOL)
and, since the fused kernel sums the pixels in the wgrad kernel's order, equal the pair's bits.
"""
import pytest
import torch

from apex_dqn_amd.ops.switches import SW

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-4
SHAPES = [(3, 0), (37, 5), (9, 16), (2, 1)]   # (images, grid): several images per workgroup with an uneven
#                                               last round, idle workgroups, one workgroup walking two images


def _lib():
    from apex_dqn_amd.ops import _lib as L
    return L.require_kernels()


def _split(x32):
    x32 = x32.to(DEV, torch.float32)
    hi = x32.to(torch.bfloat16)
    return hi, (x32 - hi.float()).to(torch.bfloat16)


def _c(t):
    return t.detach().double().cpu()


def _rel(a, b):
    a, b = _c(a), _c(b)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _empty2(*shape):
    return (torch.empty(*shape, dtype=torch.bfloat16, device=DEV),
            torch.empty(*shape, dtype=torch.bfloat16, device=DEV))


_CASES = {}


def _case(N, grid):
    """Inputs, the pair's outputs and the fp64 references of one shape (computed once)."""
    key = (N, grid)
    if key in _CASES:
        return _CASES[key]
    from apex_dqn_amd.ops import conv as C
    from apex_dqn_amd.replay.gpu_replay import to_s2d
    lib = _lib()
    g = torch.Generator(device="cpu").manual_seed(N + 5)
    raw = torch.randint(0, 256, (40, 84, 84), generator=g, dtype=torch.uint8).to(DEV)
    ring = to_s2d(raw)
    slots = torch.randint(0, 40, (N, 4), generator=g, dtype=torch.int32).to(DEV)
    dyh, dyl = _split(torch.randn(N, 9, 9, 64, generator=g))
    wh, wl = _split(torch.randn(64, 4, 4, 64, generator=g) * 0.03)
    y1 = torch.relu(torch.randn(N, 20, 20, 64, generator=g)).to(DEV, torch.bfloat16)
    # the pair: per-image dgrad kernel (not the (image, class) one), then the wgrad kernel
    cls_max = SW.conv2_dgrad_cls_max
    SW.conv2_dgrad_cls_max = 0
    try:
        dxh, dxl = _empty2(N, 20, 20, 64)
        C.conv2_dgrad_img(lib, dyh, wh, y1, dxh, grid=grid, dy_lo=dyl, w_lo=wl, out_lo=dxl)
    finally:
        SW.conv2_dgrad_cls_max = cls_max
    dw_p, db_p = torch.empty(64, 4, 8, 8, device=DEV), torch.empty(64, device=DEV)
    C.conv1_wgrad_ring(lib, C.Workspace(), dxh, ring, slots, 1 / 255.0, dw_p, db_p, grid=grid, dy_lo=dxl)
    torch.cuda.synchronize()
    # fp64: conv1's weight gradient of the joined (bit-identical) dY1 planes
    dy1 = dxh.double().cpu() + dxl.double().cpu()
    x = _c(raw[slots.long()]) / 255.0
    rdw = torch.nn.grad.conv2d_weight(x, (64, 4, 8, 8), dy1.permute(0, 3, 1, 2), stride=4)
    rdb = dy1.sum((0, 1, 2))
    _CASES[key] = dict(ring=ring, slots=slots, dyh=dyh, dyl=dyl, wh=wh, wl=wl, y1=y1, dxh=dxh, dxl=dxl,
                       dw_p=dw_p, db_p=db_p, rdw=rdw, rdb=rdb)
    return _CASES[key]


def _fused(c, grid, debug):
    from apex_dqn_amd.ops import conv as C
    N = c["dyh"].shape[0]
    dw, db = torch.empty(64, 4, 8, 8, device=DEV), torch.empty(64, device=DEV)
    dx, dxl = _empty2(N, 20, 20, 64) if debug else (None, None)
    if debug:
        dx.fill_(float("nan"))
        dxl.fill_(float("nan"))
    C.conv2_dgrad_conv1_wgrad_fused(_lib(), C.Workspace(), c["dyh"], c["dyl"], c["wh"], c["wl"], c["y1"], c["ring"],
                                    c["slots"], 1 / 255.0, dw, db, grid=grid, dx=dx, dx_lo=dxl)
    torch.cuda.synchronize()
    return dw, db, dx, dxl


@pytest.mark.parametrize("N,grid", SHAPES)
def test_dy1_bit_identical_and_grads_vs_fp64(N, grid):
    """Debug store on: the dY1 planes equal the per-image dgrad kernel's bit for bit; dW1 /
    db1 of the fused kernel AND of the pair are within TOL of fp64; with the debug store
    off the results are the same bits."""
    c = _case(N, grid)
    dw, db, dx, dxl = _fused(c, grid, True)
    assert torch.equal(dx.view(torch.int16), c["dxh"].view(torch.int16))
    assert torch.equal(dxl.view(torch.int16), c["dxl"].view(torch.int16))
    e = dict(fused_dw=_rel(dw, c["rdw"]), fused_db=_rel(db, c["rdb"]), pair_dw=_rel(c["dw_p"], c["rdw"]),
             pair_db=_rel(c["db_p"], c["rdb"]))
    print(f"N={N} grid={grid} relative error vs fp64:", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) < TOL, e
    # the k-steps take the pixels in the wgrad kernel's own order: the same bits as the pair
    assert torch.equal(dw, c["dw_p"]) and torch.equal(db, c["db_p"])
    dw0, db0, _, _ = _fused(c, grid, False)
    assert torch.equal(dw0, dw) and torch.equal(db0, db)


def _learner(B, branched, fused, monkeypatch):
    import numpy as np
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    monkeypatch.setattr(SW, "bwd_branches", branched)
    monkeypatch.setattr(SW, "conv21_bwd_fused", fused)
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
    assert L.split and L._branched == branched
    return L


@pytest.mark.parametrize("branched", [False, True])
def test_learner_step_switch_on_vs_off(monkeypatch, branched):
    """One eager B = 288 fp32 step (the smallest multiple of 32 above conv2_dgrad_cls_max)
    from the same seed with the fused kernel and with the pair: conv1's gradients agree to
    2e-4 and each is within TOL of fp64 (conv1's weight gradient of the pair's dY1 planes);
    every gradient is bit-identical."""
    from apex_dqn_amd.ops import conv as C
    B = 288
    assert B > SW.conv2_dgrad_cls_max
    res, calls = {}, []
    real = C.conv2_dgrad_conv1_wgrad_fused
    monkeypatch.setattr(C, "conv2_dgrad_conv1_wgrad_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for fused in (False, True):
        L = _learner(B, branched, fused, monkeypatch)
        L._seg1()
        L._seg2()
        torch.cuda.synchronize()
        res[fused] = {k: v.clone() for k, v in L.G.items()}
        assert len(calls) == int(fused)
        if not fused:
            dy1 = L.dY1.double().cpu() + L.dY1_lo.double().cpu()
            x = _c(L.replay.gather_frames(L.S["obs"])) * L.rt.obs_scale
            rdw = torch.nn.grad.conv2d_weight(x, (64, 4, 8, 8), dy1.permute(0, 3, 1, 2), stride=4)
            rdb = dy1.sum((0, 1, 2))
    for k in res[False]:     # conv1's included: the fused kernel sums in the pair's order
        assert torch.equal(res[False][k], res[True][k]), k
    e = dict(w1=_rel(res[True]["w1"], res[False]["w1"]), b1=_rel(res[True]["b1"], res[False]["b1"]))
    e64 = {f"{k}_{'fused' if f else 'pair'}": _rel(res[f][k].reshape(r.shape), r)
           for f in (False, True) for k, r in (("w1", rdw), ("b1", rdb))}
    print("fused vs pair:", e, "vs fp64:", {k: f"{v:.2e}" for k, v in e64.items()})
    assert max(e.values()) < 2e-4, e
    assert max(e64.values()) < TOL, e64


def test_launcher_refusals_and_backend_fallback(monkeypatch):
    """The launcher refuses C != 4, a missing lo plane and a work queue; the backend then
    (and for small batches) runs the pair instead of the fused wrapper."""
    from apex_dqn_amd.ops import _lib as L
    from apex_dqn_amd.ops import conv as C
    from apex_dqn_amd.ops.conv_sigs import Conv21BwdDesc
    from apex_dqn_amd.ops.fused_ops import HipBackend
    lib = _lib()
    c = _case(3, 0)
    ws = C.Workspace()
    slab, bslab = torch.empty(3 * 64 * 256, device=DEV), torch.empty(3 * 64, device=DEV)
    zero = torch.zeros(64, dtype=torch.uint8, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)

    def desc(**kw):
        d = Conv21BwdDesc()
        d.dy, d.dy_lo, d.w, d.w_lo = (c["dyh"].data_ptr(), c["dyl"].data_ptr(), c["wh"].data_ptr(),
                                      c["wl"].data_ptr())
        d.mask, d.wfrag, d.wfrag_ready = c["y1"].data_ptr(), C.c2d_wfrag_buffer(ws, DEV).data_ptr(), 0
        d.ring, d.slots, d.zero16 = c["ring"].data_ptr(), c["slots"].data_ptr(), zero.data_ptr()
        d.slab, d.bias_slab, d.N, d.C = slab.data_ptr(), bslab.data_ptr(), 3, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    st = L.stream_ptr()
    assert lib.apex_conv21_bwd_fused(desc(), 3, st) == 0
    assert lib.apex_conv21_bwd_fused(desc(C=1), 3, st) != 0
    assert lib.apex_conv21_bwd_fused(desc(dy_lo=None), 3, st) != 0
    assert lib.apex_conv21_bwd_fused(desc(wq=ctr.data_ptr()), 3, st) != 0
    assert lib.apex_conv21_bwd_fused(desc(), 0, st) != 0
    assert lib.apex_conv21_bwd_fused(desc(dy=c["dyh"].data_ptr() + 2), 3, st) != 0
    torch.cuda.synchronize()

    # backend: fused only above conv2_dgrad_cls_max, without a work queue, with the switch on
    calls = []
    monkeypatch.setattr(SW, "conv21_bwd_fused", True)
    monkeypatch.setattr(C, "conv2_dgrad_conv1_wgrad_fused", lambda *a, **k: calls.append("fused"))
    be = HipBackend(torch.bfloat16)
    monkeypatch.setattr(be, "conv_dgrad", lambda *a, **k: calls.append("dgrad"))
    monkeypatch.setattr(be, "conv1_wgrad_ring", lambda *a, **k: calls.append("wgrad"))
    dw, db = torch.empty(64, 4, 8, 8, device=DEV), torch.empty(64, device=DEV)

    def run(slots=c["slots"], **kw):
        del calls[:]
        args = dict(dy2_lo=c["dyl"], w2_lo=c["wl"], dy1_lo=c["dxl"])
        args.update(kw)
        be.conv2_dgrad_conv1_wgrad(c["dyh"], c["wh"], c["y1"], c["dxh"], c["ring"], slots, None, 1 / 255.0, dw, db,
                                   jobs=[], **args)
        return list(calls)

    assert run() == ["dgrad", "wgrad"]                         # 3 images <= conv2_dgrad_cls_max
    monkeypatch.setattr(SW, "conv2_dgrad_cls_max", 2)
    assert run() == ["fused"]
    assert run(dy2_lo=None, w2_lo=None, dy1_lo=None) == ["dgrad", "wgrad"]      # bf16 operands
    assert run(slots=c["slots"][:, :1].contiguous()) == ["dgrad", "wgrad"]      # C = 1
    monkeypatch.setattr(SW, "work_queue", "on")
    assert run() == ["dgrad", "wgrad"]
    monkeypatch.setattr(SW, "work_queue", "auto")
    monkeypatch.setattr(SW, "conv21_bwd_fused", False)
    assert run() == ["dgrad", "wgrad"]
