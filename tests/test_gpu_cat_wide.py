"""Wide categorical (C51) and histogram-loss heads (``Runtime.wide_atoms``, csrc/cat_wide_head.hip) on the GPU against
the fp64 torch oracle on tests/test_gpu_c51.py's fixtures (generator seed 2; tests/test_cat_wide_cpu.py lists the
problems, checks their top-2 gaps and derives ``C51_DHEAD_ATOL``, the one bound that is not ``hlg_fixtures.compare``'s
or ``test_gpu_c51._compare``'s), then the launchers, the actor head, the whole step, graph replay and the GPU loop."""
import functools

import hlg_fixtures as F
import numpy as np
import pytest
import test_gpu_c51 as C
import test_gpu_hlgauss as H
import test_gpu_qr_wide as Q
import torch
from test_cat_wide_cpu import C51_DHEAD_ATOL, EDGE, NARROW_SHAPES, RESCALED, WIDE_SHAPES, cat_torch

pytestmark = pytest.mark.gpu
DEV, VMIN, VMAX = C.DEV, C.VMIN, C.VMAX
KINDS = ["c51", "hlg"]


@pytest.fixture(autouse=True)
def _wide(monkeypatch):
    """Every head call of ``_run_hip`` of the two narrow GPU files goes through the wide launches."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    for name in ("c51_head", "hlg_head", "c51_actor_head"):
        monkeypatch.setattr(HipBackend, name, functools.partialmethod(getattr(HipBackend, name), wide=True))


def _check(kind, B, A, N, split=False, case="plain", eps=None, every=False):
    r, fx = cat_torch(kind, B, A, N, split, case, eps), C._fixture(B, A, N, split)
    h = (H._run_hip(B, A, N, split, case, rescale_eps=eps, every=every) if kind == "hlg" else
         C._run_hip(fx, A, N, *F.case_inputs(fx, case), isn=every))
    # every error in units of hlg_fixtures' tolerances, and dhead's in absolute terms
    print(kind, (B, A, N, split, case, eps), {k: f"{v:.2e}" for k, v in F.max_errors(h, r).items()})
    if kind == "hlg":
        F.compare(h, r)
    else:
        torch.testing.assert_close(h["dhead"], r["dhead"].float(), rtol=1e-4, atol=C51_DHEAD_ATOL)
        C._compare({**h, "dhead": r["dhead"].float()}, r)
    assert h["zeroed"] and (A == 1 or r["gap"] >= 1e-3)      # no near-tie in the online argmax: no sample left out
    return h, r


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", WIDE_SHAPES + NARROW_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_cat_wide_head_vs_fp64_oracle(kind, B, A, N, split):
    """(3, 2, 65): less than one row tile, one atom in the second register set, ragged column tiles; (37, 4, 101): a
    ragged row tile at the 2B boundary; (16, 18, 128): many column tiles, an edge hand-over exactly at a set boundary;
    (64, 1, 256): the dueling mean is the identity, the largest N; (64, 3, 96): a half-empty second set; (64, 4, 51)
    and (64, 3, 64): the wide path on shapes the narrow kernels are tested at.  Split (3, 2, 65) passes every optional
    argument at once; the IS statistic (max(isw) / 2 in fp64 on the same fp32 weights) and its count are exact."""
    every = split and (B, A, N) == WIDE_SHAPES[0]
    h, r = _check(kind, B, A, N, split, every=every)
    if every:
        assert r["count"] == B and h["count"] == B
        assert r["isn"] == float(C._fixture(B, A, N, True)["isw"].max().double() / C.WSCALE) and h["isn"] == r["isn"]


def test_cat_wide_rescale_instantiation(monkeypatch):
    """``cat_wide_finish_kernel<., true, .>`` at eps = 1e-3, split inputs (tests/test_gpu_c51.py's ``_run_hip`` has no
    ``rescale_eps``: it is bound to the call here)."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    _check("hlg", *RESCALED, True, eps=F.EPS)
    monkeypatch.setattr(HipBackend, "c51_head", functools.partialmethod(HipBackend.c51_head, rescale_eps=F.EPS))
    _, r = _check("c51", *RESCALED, True, eps=F.EPS)
    assert float((r["td"] - cat_torch("c51", *RESCALED, True)["td"]).abs().max()) > 0.1       # (not the plain target)


@pytest.mark.parametrize("case", F.EDGE_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_cat_wide_edge_cases(kind, case):
    """tests/test_gpu_c51.py's and tests/test_gpu_hlgauss.py's edge checks at N = 101.  sum_i d v[i] = w grad_scale
    (sum p - sum m) = 0 up to the (N + 3) fp32 roundings of the two unit sums, 104 x 2^-23 = 1.24e-5, times
    w grad_scale <= 1 / B.  Clamped onto an end, the row is one-hot (C51) or the truncated Gaussian (HL-Gauss)."""
    from apex_dqn_amd.learner.losses import hl_gauss_target
    B, A, N = EDGE
    h, r = _check(kind, B, A, N, False, case)
    assert float(h["dhead"][:, :N].sum(1).abs().max()) <= (N + 3) * 2.0 ** -23 / B
    if case in ("rew_hi", "rew_lo"):
        fx, end = C._fixture(B, A, N), VMAX if case == "rew_hi" else VMIN
        m = torch.nn.functional.one_hot(torch.full((B,), N - 1 if case == "rew_hi" else 0), N).double()
        if kind == "hlg":
            m = hl_gauss_target(torch.full((B,), end, dtype=torch.float64), VMIN, VMAX, N, F.SIGMA)
            assert 0.5 < float(m.max()) < 0.9                   # not one-hot
        torch.testing.assert_close(h["loss"], (-fx["isw"].double() * (m * r["lp"]).sum(-1)).float(), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(h["td"], (end - r["q"][torch.arange(B), fx["act"].long()]).abs().float(),
                                   rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("bad", ["N", "hidden", "null", "L"])
@pytest.mark.parametrize("kind", KINDS)
def test_cat_wide_launcher_refuses(kind, bad):
    """N = 257, a 256-wide stream, a null output and a null workspace each return hipErrorInvalidValue (1) and launch
    nothing: the outputs keep their fill."""
    from apex_dqn_amd.ops import _lib
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be, (B, A, N) = HipBackend(), (8, 2, 65)
    fx = C._fixture(B, A, N)
    t = {k: v.to(DEV) for k, v in fx.items() if isinstance(v, torch.Tensor)}
    Pon, Ptg = {k: v.to(DEV) for k, v in fx["Pon"].items()}, {k: v.to(DEV) for k, v in fx["Ptg"].items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH, dhead = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16), torch.full((B, (A + 1) * N), 7.0, device=DEV)
    a = _lib.C51WideArgs() if kind == "c51" else _lib.HlgWideArgs()
    be._head_io(a.io, t["Hon"], t["Htg"], Pon, Ptg, t["act"], t["rew"], t["gam"], t["isw"], A, 512, 1.0 / B, td, loss, dH,
                dhead, None, None, None, None)
    ws = be.qr_wide_logits(3 * B, A, N, DEV)
    a.N, a.vmin, a.vmax, a.L = 257 if bad == "N" else N, VMIN, VMAX, None if bad == "L" else ws.data_ptr()
    a.io.hidden = 256 if bad == "hidden" else 512
    if kind == "hlg":
        a.sigma_ratio = F.SIGMA
    if bad == "null":
        a.io.td_abs = None
    assert getattr(be.lib, f"apex_{kind}_wide_head")(a, _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((td == -1).all()) and bool((loss == -1).all()) and bool((dhead == 7).all()) and not bool(dH.any())


@pytest.mark.parametrize("E", [5, 64])
@pytest.mark.parametrize("N", [65, 101])
def test_cat_wide_actor_head_vs_oracle(E, N):
    """q against the fp64 q at tests/test_gpu_c51.py's actor tolerance; with eps = 0.9 the actions equal the host mirror
    of the counter RNG (replay/gpu_replay.py ``apex_uniform``, words 2 e and 2 e + 1): greedy rows and drawn rows."""
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend
    from apex_dqn_amd.replay.gpu_replay import apex_uniform
    A, fx = 4, C._fixture(64, 4, N)
    H_, P = fx["Hon"][64:64 + E].contiguous(), fx["Pon"]      # the S_t+n rows
    z = VMIN + torch.arange(N, dtype=torch.float64) * ((VMAX - VMIN) / (N - 1))
    q_ref = (TorchBackend._c51_logp(H_.double(), {k: v.double() for k, v in P.items()}, A, N, torch.float64).exp() * z).sum(-1)
    top = q_ref.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3
    q, a = torch.zeros(E, A, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV)
    HipBackend().c51_actor_head(H_.to(DEV), {k: v.to(DEV) for k, v in P.items()}, torch.full((E,), 0.9, device=DEV),
                                torch.full((1,), 3, dtype=torch.int64, device=DEV), 5, N, VMIN, VMAX, q, a)
    torch.cuda.synchronize()
    assert float((q.cpu().double() - q_ref).abs().max()) < 1e-4
    u, rr = apex_uniform(5, 3, 2 * np.arange(E)), apex_uniform(5, 3, 2 * np.arange(E) + 1)
    want = np.where(u < np.float32(0.9), np.minimum((rr * np.float32(A)).astype(np.int64), A - 1), q_ref.argmax(1).numpy())
    assert np.array_equal(a.cpu().numpy(), want) and 0 < int((u < np.float32(0.9)).sum()) < E


# tests/test_gpu_qr_wide.py's config and learner, with this head in place of the 200 quantiles
_cfg = functools.partial(Q._cfg, num_atoms=101, dist_head="hl_gauss", wide_atoms=True)
_learner = Q._learner


@pytest.mark.parametrize("dtype,extra", [("bf16", {}), ("fp32", {}), ("fp32", {"layer_norm": True, "noisy": True})])
def test_cat_wide_learner_step_hip_vs_torch_backend(dtype, extra):
    """tests/test_gpu_qr_wide.py's whole-step test and bounds under the histogram loss at N = 101, A = 4, B = 32."""
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, **extra)
    res = {}
    for be in ("hip", "torch"):
        L, _ = _learner(cfg, be, split)
        assert L.N == 101 and L.cfg.hl_gauss and L.wide_cat and L.split == split and (L.qr_L is not None) == (be == "hip")
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        res[be] = (L.td_abs.clone(), L.loss_b.clone(), L.S["idx"].clone(), L.layout.views(L.g32.clone()))
    assert torch.equal(res["hip"][2], res["torch"][2])
    for k in (0, 1):
        torch.testing.assert_close(res["hip"][k], res["torch"][k], rtol=5e-2, atol=5e-2)
    gh, gt = res["hip"][3], res["torch"][3]
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} {extra}):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


def test_cat_wide_graph_replay_is_bit_identical_to_eager():
    """A 4-update graph (replayed once) leaves the bits of four eager steps."""
    res = {}
    for graphs in (True, False):
        L, rp = _learner(_cfg(32, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000}), seed=3, fill=1)
        L.steps(4) if graphs else [L.step() for _ in range(4)]
        torch.cuda.synchronize()
        assert L.num_q_updates == 4 and (not graphs or L._multi is not None)
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.td_abs.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_cat_wide_gpu_loop_lock_step():
    """Lock step with one actor group at A = 6: the learner and the group own distinct logits workspaces."""
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = _cfg(32, A=6, log_every=20, use_graphs=True,
               learner={"min_replay_mem_size": 300, "remove_old_xp_freq": 20, "q_target_sync_freq": 25})
    out = train_frames(cfg, DEV, 20, num_envs=16, async_actors=False)
    L, groups = out["learner"], getattr(out["actors"], "groups", [out["actors"]])
    torch.cuda.synchronize()
    assert L.N == 101 and L.wide_cat and L.num_q_updates == 20 and all(g.wide_cat for g in groups)
    assert len({t.data_ptr() for t in [L.qr_L] + [g.qr_L for g in groups]}) == 1 + len(groups)
    assert bool(torch.isfinite(L.td_abs).all()) and np.isfinite(L.last_metrics()["loss"]) and L.last_metrics()["grad_norm"] > 0
    assert all(bool(torch.isfinite(g.q).all()) and 0 < float(g.q.abs().max()) <= VMAX + 1e-3 for g in groups)
