"""Wide quantile head (65..256 quantiles, csrc/qr_wide_head.hip) on the GPU: the three launches against the fp64
torch oracle on the fixtures of tests/test_gpu_qr.py (generator seed 2; tests/test_qr_wide_cpu.py checks their top-2
gaps on the CPU), the forced path at N <= 64, the launchers' refusals, the actor head, the whole step against the
torch backend, graph replay, resume and the GPU loop."""
import numpy as np
import pytest
import torch
from head_fixtures import fill_replay
from test_gpu_qr import DEV, KAPPA, WSCALE, _case_inputs, _compare, _fixture, _run_hip

pytestmark = pytest.mark.gpu

WIDE_SHAPES = [(3, 2, 65), (37, 4, 200), (16, 18, 128), (64, 1, 256), (64, 3, 96)]


def _oracle(B, A, N, split=False, case="plain", kappa=KAPPA, rescale_eps=None, emulate=False):
    """``_oracle`` of tests/test_gpu_qr.py without its top-2 gap (A = 1 has none) and with ``rescale_eps``.
    ``emulate``: the head weights as the kernel's products see them, bf16 hi + bf16 lo (2^-17 relative), everything
    else in fp64 -- the CPU emulation of the product rule.  (With hi / lo activations the kernel also drops Wlo Hlo;
    that is not emulated, so the allowance below is the smaller one.)"""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(torch.float64)
    fx = _fixture(B, A, N, split)
    rew, gam, isw = _case_inputs(fx, case)
    d = lambda t: t.double()                                             # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi) + d(lo)        # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    Pon, Ptg = {k: d(v) for k, v in fx["Pon"].items()}, {k: d(v) for k, v in fx["Ptg"].items()}
    if emulate:
        for P in (Pon, Ptg):
            for k in ("wv", "wa"):
                hi = P[k].float().bfloat16().float()
                P[k] = hi.double() + (P[k].float() - hi).bfloat16().double()
    td, loss = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    dH, dhead = torch.zeros(B, 1024, dtype=torch.float64), torch.zeros(B, (A + 1) * N, dtype=torch.float64)
    q = torch.zeros(B, A, dtype=torch.float64)
    stat = (torch.full((1,), WSCALE), torch.full((1,), -1.0, dtype=torch.float64), torch.zeros((), dtype=torch.int64))
    be.qr_head(Hon, Htg, Pon, Ptg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, kappa, 1.0 / B, td,
               loss, dH, dhead, q_out=q, isn=None if isw is None else stat, rescale_eps=rescale_eps)
    gr = {k: torch.zeros_like(v) for k, v in Pon.items()}
    be.head_wgrad(Hon, dhead, gr)
    return dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, isn=float(stat[1]), count=int(stat[2]))


def _compare_emulated(h, r, e):
    """``_compare`` with dhead's absolute bound raised to 4 x the error of the emulated product rule ``e`` against
    the fp64 oracle ``r`` on the same fixture, where that is larger.  A row with gamma = 0 (every case has them:
    the fixture's gam[::7]) has u_ij = R - theta_i for every j, so a theta_i within 1e-5 of R turns the weights'
    2^-17 into an error of g_i that no j averages out.  The other quantities keep their bounds."""
    floor = 4 * float((e["dhead"] - r["dhead"]).abs().max())
    print(f"emulated product rule: dhead err {floor / 4:.2e}; kernel {float((h['dhead'] - r['dhead']).abs().max()):.2e}")
    torch.testing.assert_close(h["dhead"], r["dhead"].float(), rtol=1e-4, atol=max(1e-7, floor))
    _compare({**h, "dhead": r["dhead"].float()}, r)


# --------------------------------------------------------- 1. kernels vs oracle
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", WIDE_SHAPES)
def test_qr_wide_head_vs_fp64_oracle(B, A, N, split):
    """(3, 2, 65): less than one row tile, one quantile in the second register set, ragged column tiles; (37, 4,
    200): a ragged row tile at the 2B boundary, the paper's N; (16, 18, 128): many column tiles; (64, 1, 256): the
    dueling mean is the identity, the largest N; (64, 3, 96): a half-empty second set.  ``_compare``'s bounds."""
    r, h = _oracle(B, A, N, split), _run_hip(B, A, N, split)
    print({k: f"{float((h[k] - r[k]).abs().max()):.2e}" for k in ("td", "loss", "dhead", "dH", "q")})
    _compare(h, r)
    assert h["zeroed"]


@pytest.mark.parametrize("B,A,N", [(64, 4, 32), (64, 18, 64)])
def test_qr_wide_forced_at_narrow_shapes(B, A, N, monkeypatch):
    """``SW.qr_wide`` sends N <= 64 through the wide launches: the shapes qr_head_kernel is tested at."""
    from apex_dqn_amd.ops.switches import SW
    monkeypatch.setattr(SW, "qr_wide", True)
    for split in (False, True):
        _compare(_run_hip(B, A, N, split), _oracle(B, A, N, split))


# ------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("case", ["rew_hi", "rew_lo", "terminal", "no_isw", "kappa"])
def test_qr_wide_edge_cases(case):
    B, A, N = 37, 4, 200
    kappa = 0.25 if case == "kappa" else KAPPA
    fx, r, h = _fixture(B, A, N), _oracle(B, A, N, False, case, kappa), _run_hip(B, A, N, False, case, kappa)
    _compare_emulated(h, r, _oracle(B, A, N, False, case, kappa, emulate=True))
    if case == "terminal":      # T_j = R for every j: the priority is |R - q(S_t)[a]|
        qa = r["q"][torch.arange(B), fx["act"].long()]
        torch.testing.assert_close(h["td"], (fx["rew"].double() - qa).abs().float(), rtol=1e-4, atol=1e-4)
    # the dueling split of the gradient: the advantage rows sum to zero over the actions
    dadv = h["dhead"][:, N:].reshape(B, A, N)
    assert float(dadv.sum(1).abs().max()) <= 4 * 2.0 ** -23 * float(h["dhead"][:, :N].abs().max())


def test_qr_wide_rescaled_with_every_optional_argument(monkeypatch):
    """q_out, the zeroed region, the lo planes, the IS weights and the IS statistic with its row count (equal to the
    oracle's exactly, as in tests/test_gpu_qr.py); then the RESCALE instantiation through the same call."""
    import functools

    from apex_dqn_amd.ops.fused_ops import HipBackend
    B, A, N = 37, 4, 200
    h = _run_hip(B, A, N, True, isn=True)
    _compare(h, _oracle(B, A, N, True))
    assert h["zeroed"] and h["count"] == B and h["isn"] == float(_fixture(B, A, N, True)["isw"].max().double() / WSCALE)
    monkeypatch.setattr(HipBackend, "qr_head", functools.partialmethod(HipBackend.qr_head, rescale_eps=1e-2))
    _compare(_run_hip(B, A, N, True), _oracle(B, A, N, True, rescale_eps=1e-2))


# ------------------------------------------------------- 3. launcher refusals
@pytest.mark.parametrize("bad", ["N", "hidden", "null"])
def test_qr_wide_launcher_refuses(bad):
    """N = 257, a 256-wide stream and a null output each return hipErrorInvalidValue (1) and launch nothing: the
    outputs keep their fill."""
    from apex_dqn_amd.ops import _lib
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be, (B, A, N) = HipBackend(), (8, 2, 65)
    fx = _fixture(B, A, N)
    t = {k: v.to(DEV) for k, v in fx.items() if isinstance(v, torch.Tensor)}
    Pon, Ptg = {k: v.to(DEV) for k, v in fx["Pon"].items()}, {k: v.to(DEV) for k, v in fx["Ptg"].items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH, dhead = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16), torch.full((B, (A + 1) * N), 7.0, device=DEV)
    a = _lib.QRWideArgs()
    be._head_io(a.io, t["Hon"], t["Htg"], Pon, Ptg, t["act"], t["rew"], t["gam"], t["isw"], A, 512, 1.0 / B, td, loss, dH,
                dhead, None, None, None, None)
    a.N, a.kappa, a.L = N, KAPPA, be.qr_wide_logits(3 * B, A, N, DEV).data_ptr()
    if bad == "N":
        a.N = 257
    elif bad == "hidden":
        a.io.hidden = 256
    else:
        a.io.td_abs = None
    assert be.lib.apex_qr_wide_head(a, _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((td == -1).all()) and bool((loss == -1).all()) and bool((dhead == 7).all()) and not bool(dH.any())


# -------------------------------------------------------------- 4. actor head
@pytest.mark.parametrize("E", [5, 64])
@pytest.mark.parametrize("N", [65, 200])
def test_qr_wide_actor_head_vs_oracle(E, N):
    """q against the fp64 q at tests/test_gpu_qr.py's actor tolerance; with eps = 0.9 the actions equal the host mirror
    of the counter RNG (replay/gpu_replay.py ``apex_uniform``, words 2 e and 2 e + 1): greedy rows and drawn rows."""
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend
    from apex_dqn_amd.replay.gpu_replay import apex_uniform
    A = 4
    fx = _fixture(64, A, N)
    H, P = fx["Hon"][64:64 + E].contiguous(), fx["Pon"]      # the S_t+n rows: top-2 gap 2.9e-3 / 4.9e-3 (fp64, CPU)
    q_ref, a_ref = torch.zeros(E, A, dtype=torch.float64), torch.zeros(E, dtype=torch.int32)
    eps, ctr = torch.full((E,), 0.9), torch.full((1,), 3, dtype=torch.int64)
    TorchBackend(torch.float64).qr_actor_head(H.double(), {k: v.double() for k, v in P.items()}, eps, ctr, 5, N,
                                              q_ref, a_ref)
    top = q_ref.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3
    q, a = torch.zeros(E, A, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV)
    HipBackend().qr_actor_head(H.to(DEV), {k: v.to(DEV) for k, v in P.items()}, eps.to(DEV), ctr.to(DEV), 5, N, q, a)
    torch.cuda.synchronize()
    assert float((q.cpu().double() - q_ref).abs().max()) < 1e-4
    e = np.arange(E)
    u, rr = apex_uniform(5, 3, 2 * e), apex_uniform(5, 3, 2 * e + 1)
    drawn = np.minimum((rr * np.float32(A)).astype(np.int64), A - 1)
    want = np.where(u < np.float32(0.9), drawn, q_ref.argmax(1).numpy())
    assert np.array_equal(a.cpu().numpy(), want) and 0 < int((u < np.float32(0.9)).sum()) < E


# -------------------------------------------------------------- 5. whole step
def _cfg(B, A=4, learner=None, **rt):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                 "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16, "Q_network_sync_freq": 10},
                                 "Learner": {"replay_sample_size": B, **(learner or {})},
                                 "Replay_Memory": {"soft_capacity": 4000},
                                 "Runtime": {"num_atoms": 200, "dist_head": "quantile", **rt}})


def _learner(cfg, backend="hip", split=False, seed=7, fill=11):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    torch.manual_seed(0)
    rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=seed)
    fill_replay(rp, 1500, A=int(cfg.env_conf.action_dim), seed=fill)      # actions inside the head's A
    return FusedNatureLearner(cfg, DEV, rp, backend=backend, split=split), rp


@pytest.mark.parametrize("dtype,extra", [("bf16", {}), ("fp32", {}), ("fp32", {"layer_norm": True, "noisy": True})])
def test_qr_wide_learner_step_hip_vs_torch_backend(dtype, extra):
    """tests/test_gpu_qr.py's whole-step test and bounds at N = 200, A = 4, B = 32; one case with LayerNorm and the
    noisy layers (whose compose launcher takes the head's shapes unchanged)."""
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, **extra)
    res = {}
    for be in ("hip", "torch"):
        L, _ = _learner(cfg, be, split)
        assert L.N == 200 and L.quantile and L.split == split
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout)
    assert torch.equal(res["hip"][2], res["torch"][2])
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} {extra}):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


def test_qr_wide_graph_replay_is_bit_identical_to_eager():
    """A 4-update graph (replayed once) leaves the bits of four eager steps."""
    res = {}
    for graphs in (True, False):
        L, rp = _learner(_cfg(32, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000}), seed=3, fill=1)
        if graphs:
            L.steps(4)
            assert L._multi is not None
        else:
            for _ in range(4):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 4
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.td_abs.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_qr_wide_resume_is_bit_identical(tmp_path):
    """Two steps, save, load into a fresh learner: the same parameters, and the checkpoint keeps the (N, 512) /
    (A N, 512) head shapes."""
    cfg = _cfg(32, use_graphs=False)
    L, _ = _learner(cfg)
    L.step()
    L.step()
    torch.cuda.synchronize()
    path = str(tmp_path / "qr200.pt")
    L.save(path)
    L2, _ = _learner(cfg, seed=9, fill=5)
    assert L2.load(path)
    for a, b in ((L.p32, L2.p32), (L.t32, L2.t32), (L.rms_v, L2.rms_v), (L.pbf, L2.pbf)):
        assert torch.equal(a, b)
    assert L2.P["wv"].shape == (200, 512) and L2.P["wa"].shape == (800, 512) and L2.num_q_updates == 2


@pytest.mark.parametrize("async_actors", [False, True])
def test_qr_wide_gpu_loop(async_actors):
    """Lock step with one actor group, and the default actor thread with its pipelined groups on their own streams:
    the learner and every group own a logits workspace."""
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = _cfg(32, A=6, log_every=20, use_graphs=True,
               learner={"min_replay_mem_size": 300, "remove_old_xp_freq": 20, "q_target_sync_freq": 25})
    out = train_frames(cfg, DEV, 20, num_envs=16, async_actors=async_actors)
    L, groups = out["learner"], getattr(out["actors"], "groups", [out["actors"]])
    torch.cuda.synchronize()
    assert L.N == 200 and L.quantile and L.num_q_updates == 20 and len(groups) == (2 if async_actors else 1)
    assert len({t.data_ptr() for t in [L.qr_L] + [g.qr_L for g in groups]}) == 1 + len(groups)
    m = L.last_metrics()
    assert bool(torch.isfinite(L.td_abs).all()) and np.isfinite(m["loss"]) and m["grad_norm"] > 0
    assert all(bool(torch.isfinite(g.q).all()) and float(g.q.abs().max()) > 0 for g in groups)
