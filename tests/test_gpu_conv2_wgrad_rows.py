"""Row-resident conv2 weight gradient (csrc/conv2_wgrad_rows.hip) against the generic
split-mode kernel it replaces at large batches (igemm_wgrad_kernel<1, 9, 81, 1, 2, 1>) and
against fp64.

The new kernel reproduces the generic kernel's arithmetic (the same splits, per tile one
accumulator chain over the 64-row steps, the same three MFMAs per step, the same pair sum), so
dW2 / db2 are the same bits; both are bounded against fp64 with the replaced kernel's own
tolerance (tests/test_gpu_split.py TOL).
"""
import pytest
import torch

from apex_dqn_amd.ops.switches import SW

DEV = torch.device("cuda", 0)
TOL = 1e-4          # tests/test_gpu_split.py TOL: relative L2 of the split-mode kernels vs fp64
# (images, target_rows; 0 = the default of ops/conv.py: 352 below 256 images, i.e. five 64-row steps)
CASES = [
    (1, 0),      # one split of 81 rows: the second 64-row step is mostly past-the-end zero rows
    (9, 0),      # 729 rows in splits of 320: the last holds 89 rows
    (9, 704),    # the second split holds 25 rows and starts inside an image
    (18, 128),   # twelve splits: every boundary and most steps straddle images, the ring wraps
    (37, 0),     # several full splits and an uneven last one
    (37, 704),
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


_INPUTS = {}


def _inputs(N):
    """Operand planes and the fp64 reference of one batch size (computed once, never changed)."""
    if N not in _INPUTS:
        g = torch.Generator(device="cpu").manual_seed(N + 17)
        dy32 = torch.randn(N, 9, 9, 64, generator=g)
        y32 = torch.relu(torch.randn(N, 20, 20, 64, generator=g))
        dyh, dyl = _split(dy32)
        yh, yl = _split(y32)
        dy64 = dyh.double().cpu() + dyl.double().cpu()
        y64 = yh.double().cpu() + yl.double().cpu()
        rdw = torch.nn.grad.conv2d_weight(y64.permute(0, 3, 1, 2), (64, 64, 4, 4), dy64.permute(0, 3, 1, 2),
                                          stride=2).permute(0, 2, 3, 1).contiguous()      # OIHW -> OHWI
        _INPUTS[N] = dict(dyh=dyh, dyl=dyl, yh=yh, yl=yl, rdw=rdw, rdb=dy64.sum((0, 1, 2)))
    return _INPUTS[N]


def _run(c, target_rows, rows_kernel):
    from apex_dqn_amd.ops import conv as C
    ws = C.Workspace()
    N = c["dyh"].shape[0]
    # NaN-filled slabs of the size conv_wgrad will ask for: an unwritten element shows
    rows = target_rows or 352
    nsplit, _ = C._splits(N * 81, rows, C._WG_TBL)
    ws.get(("wg", 64, 1024), nsplit * 64 * 1024, DEV).fill_(float("nan"))
    ws.get(("wgb", 64, 1024), nsplit * 64, DEV).fill_(float("nan"))
    dw = torch.full((64, 4, 4, 64), float("nan"), device=DEV)
    db = torch.full((64,), float("nan"), device=DEV)
    C.conv_wgrad(_lib(), ws, c["dyh"], c["yh"], 4, 2, dw, db, target_rows=target_rows, jobs=None,
                 dy_lo=c["dyl"], x_lo=c["yl"], rows_kernel=rows_kernel)
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.gpu
@pytest.mark.parametrize("N,target_rows", CASES)
def test_same_bits_as_generic_and_within_tol_of_fp64(N, target_rows):
    c = _inputs(N)
    dw_g, db_g = _run(c, target_rows, False)
    dw_r, db_r = _run(c, target_rows, True)
    e = dict(rows_dw=_rel(dw_r, c["rdw"]), rows_db=_rel(db_r, c["rdb"]), generic_dw=_rel(dw_g, c["rdw"]),
             generic_db=_rel(db_g, c["rdb"]))
    print(f"N={N} target_rows={target_rows} relative error vs fp64:", {k: f"{v:.2e}" for k, v in e.items()})
    assert torch.equal(dw_r, dw_g)
    assert torch.equal(db_r, db_g)
    assert max(e.values()) < TOL, e


@pytest.mark.gpu
def test_launcher_refuses_uncovered_problems():
    """The launcher runs only the split-mode conv2 shape without fused norm partials."""
    from apex_dqn_amd.ops import _lib as L
    from apex_dqn_amd.ops import conv as C
    lib = _lib()
    c = _inputs(1)
    slab, bslab = torch.empty(64 * 1024, device=DEV), torch.empty(64, device=DEV)
    part = torch.zeros(64, dtype=torch.float64, device=DEV)

    def desc(**kw):
        a = dict(dy=c["dyh"].data_ptr(), x=c["yh"].data_ptr(), slab=slab.data_ptr(), bias_slab=bslab.data_ptr(),
                 N=1, H=20, W=20, Cin=64, OH=9, OW=9, KH=4, KW=4, stride=2, mode=1, Co=64, Kc=1024, ldd=64,
                 rows_per_split=128, Mred=81, dy_lo=c["dyl"].data_ptr(), x_lo=c["yl"].data_ptr())
        a.update(kw)
        return C._wg_desc(**a)

    st = L.stream_ptr()
    assert lib.apex_conv2_wgrad_rows(desc(), None, None, 1, 1.0, st) == 0
    assert lib.apex_conv2_wgrad_rows(desc(x_lo=None), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv2_wgrad_rows(desc(dy_lo=None), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv2_wgrad_rows(desc(norm_part=part.data_ptr()), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv2_wgrad_rows(desc(rows_per_split=96), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv2_wgrad_rows(desc(rows_per_split=2048), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv2_wgrad_rows(desc(KH=3, KW=3, stride=1, Kc=576), None, None, 1, 1.0, st) != 0
    assert lib.apex_conv2_wgrad_rows(desc(), None, None, 2, 1.0, st) != 0
    torch.cuda.synchronize()


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
    """Three eager fp32 updates of a 24-row batch on the branched path from the same seed, with
    the row-resident kernel (threshold 0) and with the generic one: parameters, optimizer
    state and TD errors are the same bits."""
    from apex_dqn_amd.ops import conv as C
    picks, res = [], {}
    real = C.conv2_wgrad_rows_pick
    monkeypatch.setattr(C, "conv2_wgrad_rows_pick", lambda *a, **k: (picks.append(real(*a, **k)), picks[-1])[1])
    monkeypatch.setattr(SW, "conv2_wgrad_rows_min", 0)
    for on in (True, False):
        monkeypatch.setattr(SW, "conv2_wgrad_rows", on)
        del picks[:]
        L = _learner(24, monkeypatch)
        for _ in range(3):
            L.step()
        torch.cuda.synchronize()
        # conv3's and conv2's weight gradients ask once each per update; only conv2's says yes
        assert sum(picks) == (3 if on else 0) and len(picks) == 6
        res[on] = {k: getattr(L, k).clone() for k in ("p32", "rms_v", "rms_m", "td_abs")}
    for k in res[True]:
        assert torch.equal(res[True][k], res[False][k]), k


def test_gating_picks_the_rows_kernel_only_where_it_applies(monkeypatch):
    """CPU: the covered shape and mode only, whole 64-row steps within the row table, the
    switch on and the batch at or above the threshold; a forced choice overrides the switch
    and the threshold but not the coverage."""
    from apex_dqn_amd.ops import conv as C
    y1, dy2 = (512, 20, 20, 64), (512, 9, 9, 64)
    pick = C.conv2_wgrad_rows_pick
    monkeypatch.setattr(SW, "conv2_wgrad_rows", True)
    monkeypatch.setattr(SW, "conv2_wgrad_rows_min", 256)
    assert pick(y1, dy2, 4, 2, True, 704)
    assert pick((256, 20, 20, 64), (256, 9, 9, 64), 4, 2, True, 704)
    assert not pick((255, 20, 20, 64), (255, 9, 9, 64), 4, 2, True, 320)          # below the threshold
    assert not pick(y1, dy2, 4, 2, False, 704)                                    # bf16 learner
    assert not pick((512, 9, 9, 64), (512, 7, 7, 64), 3, 1, True, 384)            # conv3
    assert not pick(y1, dy2, 4, 2, True, 1088)                                    # past the row table
    assert not pick(y1, dy2, 4, 2, True, 100)                                     # not whole steps
    assert not pick((512, 20, 20, 32), dy2, 4, 2, True, 704)
    assert not pick((512, 22, 22, 64), dy2, 4, 2, True, 704)
    assert not pick(y1, (512, 9, 9, 32), 4, 2, True, 704)
    assert not pick(y1, (511, 9, 9, 64), 4, 2, True, 704)
    monkeypatch.setattr(SW, "conv2_wgrad_rows_min", 0)
    assert pick((24, 20, 20, 64), (24, 9, 9, 64), 4, 2, True, 320)
    monkeypatch.setattr(SW, "conv2_wgrad_rows", False)
    assert not pick(y1, dy2, 4, 2, True, 704)
    # forced (tests): overrides switch and threshold ...
    assert pick((1, 20, 20, 64), (1, 9, 9, 64), 4, 2, True, 320, force=True)
    monkeypatch.setattr(SW, "conv2_wgrad_rows", True)
    assert not pick(y1, dy2, 4, 2, True, 704, force=False)
    # ... but not the coverage
    with pytest.raises(ValueError):
        pick(y1, dy2, 4, 2, False, 704, force=True)
