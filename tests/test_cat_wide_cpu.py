"""``Runtime.wide_atoms`` (categorical / hl_gauss heads with up to 256 atoms, csrc/cat_wide_head.hip) without a GPU: the
key's validation, the shipped config, one inline torch step at N = 101, and the problems, the fp64 C51 oracle and the
C51 ``dhead`` bound that tests/test_gpu_cat_wide.py uses."""
import functools
import os

import hlg_fixtures as F
import pytest
import torch
from test_gpu_c51 import VMAX, VMIN, WSCALE, _fixture

WIDE_SHAPES = [(3, 2, 65), (37, 4, 101), (16, 18, 128), (64, 1, 256), (64, 3, 96)]
NARROW_SHAPES = [(64, 4, 51), (64, 3, 64)]      # the wide path forced onto shapes the narrow kernels are tested at
EDGE, RESCALED = (8, 4, 101), (37, 4, 101)
# Every C51 head problem the GPU file runs: (B, A, N, split, case, rescale_eps)
C51_PROBLEMS = ([(*s, split, "plain", None) for s in WIDE_SHAPES + NARROW_SHAPES for split in (False, True)]
                + [(*EDGE, False, case, None) for case in F.EDGE_CASES] + [(*RESCALED, True, "plain", F.EPS)])
# C51's dhead: tests/test_gpu_c51.py's atol of 1e-7 is below what the references themselves keep at these shapes (b_j
# in fp32 at delta = 20 / (N - 1); the wide path's head weights as bf16 hi + lo, 2^-17 relative).  Largest absolute
# dhead error against the fp64 oracle over C51_PROBLEMS, measured on the CPU (test_c51_dhead_bound re-measures and
# prints them): the fp32 torch backend / the fp64 oracle on the weights rounded to bf16 hi + lo, by (B, A, N) --
# (3, 2, 65) 3.3e-7 / 1.1e-7, (37, 4, 101) 7.3e-8 / 3.8e-8 (rescaled 8.7e-8 / 3.6e-8), (16, 18, 128) 3.1e-8 / 3.2e-8,
# (64, 1, 256) 2.0e-7 / 7.7e-9, (64, 3, 96) 7.0e-8 / 1.6e-8, (64, 4, 51) 1.2e-8 / 1.7e-8, (64, 3, 64) 2.7e-8 / 1.6e-8,
# the edge cases at (8, 4, 101) 2.5e-7 / 1.6e-7; dhead carries grad_scale = 1 / B, so the small batches lead
C51_DHEAD_ERR = {"fp32": 3.3e-7, "emulated": 1.6e-7}
C51_DHEAD_ATOL = 1.4e-6     # 4 x the larger, 1.32e-6, rounded up (never below 1e-7)


@functools.lru_cache(maxsize=None)
def cat_torch(kind, B, A, N, split=False, case="plain", eps=None, dtype=torch.float64, emulate=False):
    """``hlg_fixtures.run_torch`` for either kind ("c51": ``TorchBackend.c51_head``, "hlg": ``hlg_head`` at
    ``F.SIGMA``) on tests/test_gpu_c51.py's fixture, A = 1 included (no top-2 gap there).  ``emulate``: the head
    weights as the wide path's MFMAs see them (bf16 hi + lo), everything else in ``dtype``."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be, fx = TorchBackend(dtype), _fixture(B, A, N, split)
    rew, gam, isw = F.case_inputs(fx, case)
    d = lambda t: t.to(dtype)                                            # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi.double() + lo.double())     # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])

    def hilo(k, v):
        hi = v.bfloat16().float()
        return d(hi.double() + (v - hi).bfloat16().double()) if emulate and k in ("wv", "wa") else d(v)
    Pon, Ptg = {k: hilo(k, v) for k, v in fx["Pon"].items()}, {k: hilo(k, v) for k, v in fx["Ptg"].items()}
    td, loss, dH, dhead, q = (torch.zeros(*s, dtype=dtype) for s in ((B,), (B,), (B, 1024), (B, (A + 1) * N), (B, A)))
    stat = (torch.full((1,), WSCALE), torch.full((1,), -1.0, dtype=torch.float64), torch.zeros((), dtype=torch.int64))
    op, own = (be.c51_head, ()) if kind == "c51" else (be.hlg_head, (F.SIGMA,))
    op(Hon, Htg, Pon, Ptg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, VMIN, VMAX, *own, 1.0 / B,
       td, loss, dH, dhead, q_out=q, isn=None if isw is None else stat, rescale_eps=eps)
    gr = {k: torch.zeros_like(v) for k, v in Pon.items()}
    be.head_wgrad(Hon, dhead, gr)
    zs = VMIN + torch.arange(N, dtype=dtype) * ((VMAX - VMIN) / (N - 1))
    top = (be._c51_logp(Hon[B:2 * B], Pon, A, N, dtype).exp() * zs).sum(-1).topk(min(A, 2), dim=1).values
    return dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, isn=float(stat[1]), count=int(stat[2]),
                gap=float((top[:, 0] - top[:, -1]).min()) if A > 1 else float("inf"),       # A = 1 has no gap
                lp=be._c51_logp(Hon[:B], Pon, A, N, dtype)[torch.arange(B), fx["act"].long()])


def _cfg(**rt):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": 8}, "Runtime": rt})


@pytest.mark.parametrize("kind", ["categorical", "hl_gauss"])
def test_key_validation_and_round_trip(kind):
    from apex_dqn_amd.config import ApexConfig
    for n in (51, 65, 256):
        cfg = _cfg(num_atoms=n, dist_head=kind, wide_atoms=True)
        assert cfg.wide_categorical and ApexConfig.from_dict(cfg.to_dict()).Runtime.wide_atoms is True
    assert not _cfg(num_atoms=51, dist_head=kind).wide_categorical
    assert not _cfg(num_atoms=200, dist_head="quantile", wide_atoms=True).wide_categorical      # accepted, no effect
    for bad in (dict(num_atoms=257, dist_head=kind), dict(num_atoms=1), dict(num_atoms=32, dist_head="implicit")):
        with pytest.raises(ValueError, match="wide_atoms" if bad["num_atoms"] < 257 else "num_atoms"):
            _cfg(wide_atoms=True, **bad)
    with pytest.raises(ValueError, match="num_atoms.*wide_atoms"):      # off: 65 is refused, and the message names the key
        _cfg(num_atoms=65, dist_head=kind)


def test_shipped_config_and_one_inline_torch_step():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    from head_fixtures import fill_replay
    rt = ApexConfig.load(os.path.join(os.path.dirname(__file__), "..", "configs", "pong_1gpu_hlgauss101.json")).Runtime
    assert (rt.num_atoms, rt.dist_head, rt.wide_atoms) == (101, "hl_gauss", True)
    torch.manual_seed(0)
    rp = GpuReplayShard(400, 400, 500, 4, device="cpu", seed=7)
    fill_replay(rp, 300, A=4, seed=11)
    L = FusedNatureLearner(_cfg(num_atoms=101, dist_head="hl_gauss", wide_atoms=True, use_graphs=False), "cpu", rp)
    p0 = L.p32.clone()
    L.step()
    assert L.N == 101 and L.wide_cat and L.qr_L is None and L.P["wa"].shape == (404, 512)
    assert bool(torch.isfinite(L.td_abs).all()) and not torch.equal(L.p32, p0)


def test_c51_dhead_bound():
    """The table behind ``C51_DHEAD_ATOL``; and no near-tie in the online argmax of any problem."""
    worst = {"fp32": 0.0, "emulated": 0.0}
    for prob in C51_PROBLEMS:
        r = cat_torch("c51", *prob)
        assert r["gap"] >= 1e-3, (prob, r["gap"])
        err = {"fp32": cat_torch("c51", *prob, dtype=torch.float32), "emulated": cat_torch("c51", *prob, emulate=True)}
        err = {k: float((v["dhead"].double() - r["dhead"]).abs().max()) for k, v in err.items()}
        print(prob, f"gap {r['gap']:.2e}", {k: f"{v:.2e}" for k, v in err.items()})
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("largest:", worst)
    assert all(worst[k] <= 1.1 * C51_DHEAD_ERR[k] for k in worst), worst
    assert C51_DHEAD_ATOL >= max(1e-7, 4 * max(worst.values()))
