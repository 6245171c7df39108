"""Quantile-regression (QR-DQN) head on the GPU: csrc/qr_head.hip against the fp64 torch oracle
(``TorchBackend.qr_head`` / ``qr_actor_head`` on fp64 inputs), the whole step against the
torch backend, graph capture, and the GPU loop with a quantile learner and actor group."""
import functools

import numpy as np
import pytest
import torch
from head_fixtures import fill_replay, split_planes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KAPPA = 1.0


# --------------------------------------------------------------------- fixture
@functools.lru_cache(maxsize=None)
def _fixture(B, A, N, split=False):
    """Inputs (CPU) of one head problem, drawn as tests/test_gpu_c51.py draws them: generator
    seed 2, the order Hon, Htg, online head, target head, act, rew, gam, isw."""
    g = torch.Generator().manual_seed(2)
    Hon = torch.relu(torch.randn(2 * B, 1024, generator=g))
    Htg = torch.relu(torch.randn(B, 1024, generator=g))

    def P():
        return {"wv": torch.randn(N, 512, generator=g) * 0.05, "bv": torch.randn(N, generator=g),
                "wa": torch.randn(A * N, 512, generator=g) * 0.05, "ba": torch.randn(A * N, generator=g)}
    Pon, Ptg = P(), P()
    act = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    rew = torch.randn(B, generator=g) * 3
    gam = torch.full((B,), 0.97)
    gam[::7] = 0.0
    isw = torch.rand(B, generator=g)
    if split:
        (Hon, Hon_lo), (Htg, Htg_lo) = split_planes(Hon), split_planes(Htg)
    else:
        Hon, Htg, Hon_lo, Htg_lo = Hon.to(torch.bfloat16), Htg.to(torch.bfloat16), None, None
    return dict(Hon=Hon, Htg=Htg, Hon_lo=Hon_lo, Htg_lo=Htg_lo, Pon=Pon, Ptg=Ptg, act=act, rew=rew, gam=gam, isw=isw)


WSCALE = 2.0     # the sampler's factor handed to the IS statistic (a power of two: the division is exact)


@functools.lru_cache(maxsize=None)
def _oracle(B, A, N, split=False, case="plain", kappa=KAPPA):
    """fp64 CPU oracle on the joined activations of ``_fixture(B, A, N, split)`` under an edge
    ``case`` (computed once per problem, shared, never modified): (td, loss, dH, dhead, q, head
    gradients, smallest top-2 gap of the online next-state q, the isw used, the IS statistic and row count)."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(torch.float64)
    fx = _fixture(B, A, N, split)
    rew, gam, isw = _case_inputs(fx, case)
    d = lambda t: t.double()                                             # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi) + d(lo)        # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    Pon, Ptg = {k: d(v) for k, v in fx["Pon"].items()}, {k: d(v) for k, v in fx["Ptg"].items()}
    td, loss = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    dH = torch.zeros(B, 1024, dtype=torch.float64)
    dhead = torch.zeros(B, (A + 1) * N, dtype=torch.float64)
    q = torch.zeros(B, A, dtype=torch.float64)
    stat = (torch.full((1,), WSCALE), torch.full((1,), -1.0, dtype=torch.float64), torch.zeros((), dtype=torch.int64))
    be.qr_head(Hon, Htg, Pon, Ptg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, kappa,
               1.0 / B, td, loss, dH, dhead, q_out=q, isn=None if isw is None else stat)
    gr = {k: torch.zeros_like(v) for k, v in Pon.items()}
    be.head_wgrad(Hon, dhead, gr)
    qn = be._qr_theta(Hon[B:2 * B], Pon, A, N, torch.float64).mean(-1)
    top = qn.topk(2, dim=1).values
    th_t = be._qr_theta(Hon[:B], Pon, A, N, torch.float64)[torch.arange(B), fx["act"].long()]
    a_star = qn.argmax(1)
    th_g = be._qr_theta(Htg[:B], Ptg, A, N, torch.float64)[torch.arange(B), a_star]
    return dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, gap=float((top[:, 0] - top[:, 1]).min()),
                th=th_t, th_target=th_g, isn=float(stat[1]), count=int(stat[2]))


def _case_inputs(fx, case):
    B = fx["act"].shape[0]
    rew, gam, isw = fx["rew"], fx["gam"], fx["isw"]
    if case == "rew_hi":
        rew = torch.full((B,), 25.0)
    elif case == "rew_lo":
        rew = torch.full((B,), -25.0)
    elif case == "terminal":
        gam = torch.zeros(B)
    elif case == "no_isw":
        isw = None
    else:
        assert case in ("plain", "kappa"), case
    return rew, gam, isw


def _run_hip(B, A, N, split=False, case="plain", kappa=KAPPA, isn=False):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be = HipBackend()
    fx = _fixture(B, A, N, split)
    rew, gam, isw = _case_inputs(fx, case)
    dev = lambda t: None if t is None else t.to(DEV)                     # noqa: E731
    Hon, Htg, Hon_lo, Htg_lo = dev(fx["Hon"]), dev(fx["Htg"]), dev(fx["Hon_lo"]), dev(fx["Htg_lo"])
    Pon, Ptg = {k: dev(v) for k, v in fx["Pon"].items()}, {k: dev(v) for k, v in fx["Ptg"].items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16)
    dH_lo = torch.zeros_like(dH) if split else None
    dhead = torch.full((B, (A + 1) * N), 7.0, device=DEV)
    q = torch.zeros(B, A, device=DEV)
    gr = {k: torch.full_like(v, 3.0) for k, v in Pon.items()}
    flat = torch.full((sum(v.numel() for v in gr.values()),), 3.0, device=DEV)      # zeroed by the head launch
    o = 0
    for k in ("wv", "bv", "wa", "ba"):
        gr[k] = flat[o:o + gr[k].numel()].view(gr[k].shape)
        o += gr[k].numel()
    stat = (torch.full((1,), WSCALE, device=DEV), torch.full((1,), -1.0, dtype=torch.float64, device=DEV),
            torch.zeros((), dtype=torch.int64, device=DEV))
    be.qr_head(Hon, Htg, Pon, Ptg, dev(fx["act"]), dev(rew), dev(gam), dev(isw), N, kappa, 1.0 / B, td, loss,
               dH, dhead, q_out=q, zero=flat, lo=(Hon_lo, Htg_lo, dH_lo) if split else None,
               isn=stat if isn else None)
    torch.cuda.synchronize()
    zeroed = bool((flat == 0).all())
    be.head_wgrad(Hon, dhead, gr, Hon_lo=Hon_lo)
    torch.cuda.synchronize()
    dHj = dH.double() + (dH_lo.double() if split else 0.0)
    return dict(td=td.cpu(), loss=loss.cpu(), dH=dHj.cpu(), dhead=dhead.cpu(), q=q.cpu(),
                g={k: v.cpu() for k, v in gr.items()}, zeroed=zeroed, isn=float(stat[1].cpu()), count=int(stat[2].cpu()))


def _compare(h, r):
    """The tolerances of ``_compare`` in tests/test_gpu_c51.py."""
    f = lambda t: t.float()                                              # noqa: E731
    torch.testing.assert_close(h["td"], f(r["td"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(h["loss"], f(r["loss"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(f(h["dH"]), f(r["dH"]), rtol=1e-2, atol=1e-6)
    torch.testing.assert_close(h["dhead"], f(r["dhead"]), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(h["q"], f(r["q"]), rtol=1e-4, atol=1e-4)
    for k in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(h["g"][k], f(r["g"][k]), rtol=1e-3, atol=1e-6)


# --------------------------------------------------------- 1. kernel vs oracle
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", [(64, 4, 32), (64, 18, 64), (64, 6, 21), (64, 3, 51), (64, 2, 2), (5, 4, 32),
                                   (3, 2, 2)])
def test_qr_head_kernel_vs_fp64_oracle(B, A, N, split):
    """bf16 single plane and split hi / lo inputs (built from fp32 activations; the oracle
    works on the joined values).  B = 5: not a multiple of the samples per block.  The
    fixture's smallest top-2 gap of the online next-state q (fp64, measured on the CPU) is
    4.3e-3, 1.8e-3, 4.3e-3, 1.6e-3 and 3.5e-1 at the B = 64 shapes in this order, in both
    input modes: no near-tie, every sample is compared.  (3, 2, 2): a block whose second sample
    is past the batch in a head with fewer weight-row tasks (4) than waves; generator seed 2 as
    everywhere, gap 5.0e-1 in both input modes."""
    r = _oracle(B, A, N, split)
    if B != 5:
        assert r["gap"] >= 1e-3, r["gap"]
    h = _run_hip(B, A, N, split)
    print(f"B {B} A {A} N {N} split {split}: oracle gap {r['gap']:.3e}, "
          f"td err {float((h['td'] - r['td']).abs().max()):.2e}, loss err {float((h['loss'] - r['loss']).abs().max()):.2e}, "
          f"dhead err {float((h['dhead'] - r['dhead']).abs().max()):.2e}")
    _compare(h, r)


def test_qr_head_every_optional_argument_at_once():
    """q_out, the zeroed region, the three lo planes, the IS weights and the IS statistic with its output and
    its row count, all given: every member of the argument block the launch passes is read or written through,
    so a member at the wrong offset shows as a wrong number.  Two blocks, the second with one live row; the
    smallest head (N = 2).  The statistic is max(isw) / 2 formed in fp64 from the same fp32 weights, and the
    count an integer: both equal the oracle's exactly."""
    B, A, N = 3, 3, 2           # B = DIST_SPB + 1 (csrc/dist_head.h)
    fx = _fixture(B, A, N, True)
    r = _oracle(B, A, N, True)
    assert r["gap"] >= 1e-3, r["gap"]
    h = _run_hip(B, A, N, True, isn=True)
    _compare(h, r)
    assert h["zeroed"]
    assert r["count"] == B and h["count"] == r["count"]
    assert r["isn"] == float(fx["isw"].max().double() / WSCALE) and h["isn"] == r["isn"]


# ------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("case", ["rew_hi", "rew_lo", "terminal", "no_isw", "kappa"])
def test_qr_head_edge_cases(case):
    """All-terminal batches, |u| > kappa everywhere (rew = +-25), weights off, kappa = 0.25."""
    B, A, N = 8, 4, 32
    fx = _fixture(B, A, N)
    kappa = 0.25 if case == "kappa" else KAPPA
    r = _oracle(B, A, N, False, case, kappa)
    h = _run_hip(B, A, N, False, case, kappa)
    _compare(h, r)
    w = torch.ones(B, dtype=torch.float64) if case == "no_isw" else fx["isw"].double()
    tau = (2 * torch.arange(N, dtype=torch.float64) + 1) / (2 * N)
    if case in ("rew_hi", "rew_lo"):
        # every |u| > kappa, one sign: the gradient is -w gs (tau_i - 1{u < 0}) in the oracle, exactly
        u = (25.0 if case == "rew_hi" else -25.0) + fx["gam"].double()[:, None, None] * r["th_target"][:, None, :] \
            - r["th"][:, :, None]
        assert float(u.abs().min()) > KAPPA and bool(((u > 0) == (case == "rew_hi")).all())
        g_ref = -w[:, None] * (1.0 / B) * (tau - (0.0 if case == "rew_hi" else 1.0))[None, :]
        torch.testing.assert_close(r["dhead"][:, :N], g_ref, rtol=1e-12, atol=0)
        torch.testing.assert_close(h["dhead"][:, :N], g_ref.float(), rtol=1e-4, atol=1e-7)
    if case == "terminal":
        # T_j = R for every j: the priority is |R - q(S_t)[a]|
        qa = r["q"][torch.arange(B), fx["act"].long()]
        torch.testing.assert_close(h["td"], (fx["rew"].double() - qa).abs().float(), rtol=1e-4, atol=1e-4)
    # the dueling split of the gradient: the advantage rows sum to zero over the actions
    dadv = h["dhead"][:, N:].reshape(B, A, N)
    assert float(dadv.sum(1).abs().max()) <= 4 * 2.0 ** -23 * float(h["dhead"][:, :N].abs().max())


# -------------------------------------------------------------- 3. actor head
def test_qr_actor_head_vs_oracle():
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend
    E, A, N = 37, 6, 32
    fx = _fixture(64, A, N)
    H = fx["Hon"][:E]
    P = fx["Pon"]
    q_ref, a_ref = torch.zeros(E, A, dtype=torch.float64), torch.zeros(E, dtype=torch.int32)
    eps, ctr = torch.zeros(E), torch.zeros(1, dtype=torch.int64)
    TorchBackend(torch.float64).qr_actor_head(H.double(), {k: v.double() for k, v in P.items()}, eps, ctr, 5, N,
                                              q_ref, a_ref)
    top = q_ref.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3          # 5.0e-3 (fp64, measured on the CPU)
    q, a = torch.zeros(E, A, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV)
    be = HipBackend()
    Pd = {k: v.to(DEV) for k, v in P.items()}
    be.qr_actor_head(H.to(DEV), Pd, eps.to(DEV), ctr.to(DEV), 5, N, q, a)
    torch.cuda.synchronize()
    assert float((q.cpu().double() - q_ref).abs().max()) < 1e-4
    assert torch.equal(a.cpu(), q_ref.argmax(1).to(torch.int32))
    # the same counter-RNG words as the scalar actor head: with eps = 1 both draw the same actions
    one = torch.ones(E, device=DEV)
    a1, a2 = torch.zeros_like(a), torch.zeros_like(a)
    c3 = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    be.qr_actor_head(H.to(DEV), Pd, one, c3, 9, N, q, a1)
    Ps = {"wv": P["wv"][0].contiguous().to(DEV), "bv": P["bv"][:1].contiguous().to(DEV),
          "wa": P["wa"][:A].contiguous().to(DEV), "ba": P["ba"][:A].contiguous().to(DEV)}
    be.actor_head(H.to(DEV), Ps, one, c3, 9, torch.zeros(E, A, device=DEV), a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and len(set(a1.tolist())) > 1


# -------------------------------------------------------------- 4. whole step
def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"num_atoms": 32, "dist_head": "quantile", **rt}})


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_qr_learner_step_hip_vs_torch_backend(dtype):
    """tests/test_gpu_c51.py test_c51_learner_step_hip_vs_torch_backend with the quantile head
    (32 quantiles) at B = 32, in the bf16-operand mode and the fp32 (split) mode, with that
    test's bounds and its clip-norm identity."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.N == 32 and L.quantile and L.split == split
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, float(L.gnorm), gn)
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout)
    assert torch.equal(res["hip"][2], res["torch"][2])
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} HIP step vs the torch backend):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


# ------------------------------------------------------------------ 5. graphs
def test_qr_graph_steps_match_eager_steps():
    """steps(8) replaying two 4-update graphs == 8 eager step() calls of a twin learner; the
    one-update graph matches the eager update (as tests/test_gpu_c51.py checks for C51)."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res = {}
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, lr_warmup_steps=3, lr_decay_steps=6, lr_end=1e-5,
                   learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        u0 = L.update_index()
        if graphs:
            L.steps(8)
            assert L._multi is not None
        else:
            for _ in range(8):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 8 and L.update_index() - u0 == 8
        if graphs:
            assert L.graph_matches_eager() is True
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.S["idx"].clone())
    assert torch.equal(res[True][3], res[False][3])
    for a, b in zip(res[True][:3], res[False][:3]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------- 6. GPU loop
def test_qr_gpu_loop_lock_step():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 20, "q_target_sync_freq": 25},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 20, "use_graphs": True, "num_atoms": 32,
                                            "dist_head": "quantile"}})
    out = train_frames(cfg, DEV, 40, num_envs=16, async_actors=False)
    L, rp = out["learner"], out["replay"]
    torch.cuda.synchronize()
    assert L.N == 32 and L.quantile and L.num_q_updates == 40
    assert out["actors"].inserted >= 300 + 16 * 20           # inserts kept flowing beside the 40 updates
    live = rp.leaf[rp.leaf != 0]
    assert bool((live > 0).all())
    assert live.numel() >= 300 and bool(torch.isfinite(live).all())
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
    q = out["actors"].q
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all()) and float(q.abs().max()) > 0
