"""Munchausen-DQN target on the GPU: csrc/mdqn_head.hip against the fp64 torch oracle
(``TorchBackend.mdqn_head`` on fp64 inputs), the sampler's second S_t destination, the whole step
against the torch backend, graph capture, resume, and the GPU loop."""
import functools
import math

import numpy as np
import pytest
import torch
from head_fixtures import fill_replay, split_planes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ALPHA, TAU, CLIP, KAPPA = 0.9, 0.03, -1.0, 1.0


# --------------------------------------------------------------------- fixture
@functools.lru_cache(maxsize=None)
def _fixture(B, A, split=False):
    """Inputs (CPU) of one head problem: Hon [B, 1024] (online S_t), Htg [2B, 1024] (target S_t+n, then
    target S_t), both heads, act, rew, gam (every 7th terminal), isw."""
    g = torch.Generator().manual_seed(2)
    Hon = torch.relu(torch.randn(B, 1024, generator=g))
    Htg = torch.relu(torch.randn(2 * B, 1024, generator=g))

    def P():
        return {"wv": torch.randn(512, generator=g) * 0.05, "bv": torch.randn(1, generator=g),
                "wa": torch.randn(A, 512, generator=g) * 0.05, "ba": torch.randn(A, generator=g)}
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


WSCALE = 2.0     # the sampler's factor handed to the oracle's IS statistic (a power of two: the division is exact)
CASES = ("plain", "terminal", "no_isw", "equal_q", "huge_gaps", "alpha0", "mse", "tau1")


def _case_inputs(fx, case):
    """(rew, gam, isw, target head, alpha, tau, huber) of an edge ``case``."""
    B, A = fx["act"].shape[0], fx["Ptg"]["wa"].shape[0]
    gam, isw, Ptg = fx["gam"], fx["isw"], fx["Ptg"]
    alpha, tau, huber = ALPHA, TAU, True
    if case == "terminal":
        gam = torch.zeros(B)
    elif case == "no_isw":
        isw = None
    elif case == "equal_q":          # no advantage: every q of the target net equals its value
        Ptg = dict(Ptg, wa=torch.zeros(A, 512), ba=torch.full((A,), 0.3))
    elif case == "huge_gaps":        # action gaps ~ 100 = 3,333 tau: every non-max exp underflows (fp32 and fp64)
        Ptg = dict(Ptg, ba=Ptg["ba"] + 100.0 * torch.arange(A, dtype=torch.float32))
    elif case == "alpha0":
        alpha = 0.0
    elif case == "mse":
        huber = False
    elif case == "tau1":
        tau = 1.0
    else:
        assert case == "plain", case
    return fx["rew"], gam, isw, Ptg, alpha, tau, huber


@functools.lru_cache(maxsize=None)
def _oracle(B, A, split=False, case="plain"):
    """fp64 CPU oracle on the joined (rounded) activations of ``_fixture(B, A, split)`` under an edge
    ``case``: computed once per problem, shared, never modified."""
    from apex_dqn_amd.learner.losses import tau_log_policy
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(torch.float64)
    fx = _fixture(B, A, split)
    rew, gam, isw, Ptg, alpha, tau, huber = _case_inputs(fx, case)
    d = lambda t: t.double()                                             # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi) + d(lo)        # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    Pon, Ptg = {k: d(v) for k, v in fx["Pon"].items()}, {k: d(v) for k, v in Ptg.items()}
    td, loss = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    dH = torch.zeros(B, 1024, dtype=torch.float64)
    dhead = torch.zeros(B, A + 1, dtype=torch.float64)
    q = torch.zeros(B, A, dtype=torch.float64)
    aux = torch.zeros(B, 2, dtype=torch.float64)
    stat = (torch.full((1,), WSCALE), torch.full((1,), -1.0, dtype=torch.float64), torch.zeros((), dtype=torch.int64))
    be.mdqn_head(Hon, Htg, Pon, Ptg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), huber, KAPPA, alpha,
                 tau, CLIP, 1.0 / B, td, loss, dH, dhead, q_out=q, aux=aux, isn=None if isw is None else stat)
    # the head gradients of TorchBackend.head_wgrad, in fp64
    gr = {"wv": dhead[:, 0] @ Hon[:, :512], "bv": dhead[:, 0].sum().view(1), "wa": dhead[:, 1:].t() @ Hon[:, 512:],
          "ba": dhead[:, 1:].sum(0)}

    def q_of(h, P):
        a = h[:, 512:] @ P["wa"].t() + P["ba"]
        return (h[:, :512] @ P["wv"] + P["bv"])[:, None] + a - a.mean(1, keepdim=True)
    g1, g0 = q_of(Htg[:B], Ptg), q_of(Htg[B:], Ptg)
    tl = tau_log_policy(g0, tau).gather(1, fx["act"].long()[:, None]).squeeze(1)
    return dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, aux=aux, g=gr, tl=tl, g0=g0, g1=g1, isn=float(stat[1]),
                count=int(stat[2]))


def _run_hip(B, A, split=False, case="plain", isn=None, q_out=True):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be = HipBackend()
    fx = _fixture(B, A, split)
    rew, gam, isw, Ptg, alpha, tau, huber = _case_inputs(fx, case)
    dev = lambda t: None if t is None else t.to(DEV)                     # noqa: E731
    Hon, Htg, Hon_lo, Htg_lo = dev(fx["Hon"]), dev(fx["Htg"]), dev(fx["Hon_lo"]), dev(fx["Htg_lo"])
    Pon, Ptg = {k: dev(v) for k, v in fx["Pon"].items()}, {k: dev(v) for k, v in Ptg.items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16)
    dH_lo = torch.zeros_like(dH) if split else None
    dhead = torch.full((B, A + 1), 7.0, device=DEV)
    q = torch.zeros(B, A, device=DEV)
    aux = torch.full((B, 2), 5.0, device=DEV)
    flat = torch.full((sum(v.numel() for v in Pon.values()),), 3.0, device=DEV)      # zeroed by the head launch
    gr, o = {}, 0
    for k in ("wv", "bv", "wa", "ba"):
        gr[k] = flat[o:o + Pon[k].numel()].view(Pon[k].shape)
        o += Pon[k].numel()
    be.mdqn_head(Hon, Htg, Pon, Ptg, dev(fx["act"]), dev(rew), dev(gam), dev(isw), huber, KAPPA, alpha, tau, CLIP,
                 1.0 / B, td, loss, dH, dhead, q_out=q if q_out else None, aux=aux, zero=flat,
                 lo=(Hon_lo, Htg_lo, dH_lo) if split else None, isn=isn)
    torch.cuda.synchronize()
    zeroed = flat.clone()
    be.head_wgrad(Hon, dhead, gr, Hon_lo=Hon_lo)
    torch.cuda.synchronize()
    dHj = dH.double() + (dH_lo.double() if split else 0.0)
    return dict(td=td.cpu(), loss=loss.cpu(), dH=dHj.cpu(), dhead=dhead.cpu(), q=q.cpu(), aux=aux.cpu(),
                g={k: v.cpu() for k, v in gr.items()}, zeroed=zeroed.cpu())


def _compare(h, r):
    """The tolerances of ``_compare`` in tests/test_gpu_qr.py for td, loss, dH, dhead, q and the head
    gradients; aux at td's."""
    f = lambda t: t.float()                                              # noqa: E731
    print(" ".join(f"{k} err {float((h[k].double() - r[k]).abs().max()):.2e}" for k in ("td", "loss", "dH", "dhead", "q",
                                                                                      "aux")))
    torch.testing.assert_close(h["td"], f(r["td"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(h["loss"], f(r["loss"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(f(h["dH"]), f(r["dH"]), rtol=1e-2, atol=1e-6)
    torch.testing.assert_close(h["dhead"], f(r["dhead"]), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(h["q"], f(r["q"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(h["aux"], f(r["aux"]), rtol=1e-4, atol=1e-4)
    for k in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(h["g"][k], f(r["g"][k]), rtol=1e-3, atol=1e-6)
    for v in h.values():
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all())


# --------------------------------------------------------- 1. kernel vs oracle
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A", [(5, 2), (33, 4), (33, 6), (7, 9), (7, 18)])
def test_mdqn_head_kernel_vs_fp64_oracle(B, A, split):
    """bf16 single plane and split hi / lo inputs; the oracle works on the joined values.  A <= 8 runs the
    register instantiation (MAXA = 8), A = 9 and 18 the HEAD_MAXA one; one block per sample."""
    r = _oracle(B, A, split)
    h = _run_hip(B, A, split)
    _compare(h, r)
    assert bool((h["zeroed"] == 0).all())
    assert bool((h["aux"][:, 0] <= 0).all()) and bool((h["aux"][:, 0] >= ALPHA * CLIP).all())


def test_mdqn_head_every_optional_argument_at_once():
    """q_out, aux, the zeroed region, the three lo planes, the IS weights and the IS statistic with its output
    and its row count, all given: every member of the argument block the launch passes is read or written
    through, so a member at the wrong offset shows as a wrong number.  Two blocks (one per sample).  The
    statistic is max(isw) / 2 formed in fp64 from the same fp32 weights, and the count an integer: both equal
    the oracle's exactly."""
    B, A = 2, 3
    fx = _fixture(B, A, True)
    r = _oracle(B, A, True)
    isn = (torch.full((1,), WSCALE, device=DEV), torch.full((1,), -1.0, dtype=torch.float64, device=DEV),
           torch.zeros((), dtype=torch.int64, device=DEV))
    h = _run_hip(B, A, True, isn=isn)
    _compare(h, r)
    assert bool((h["zeroed"] == 0).all())
    assert r["count"] == B and int(isn[2]) == r["count"]
    assert r["isn"] == float(fx["isw"].max().double() / WSCALE) and float(isn[1]) == r["isn"]


# ------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("case", CASES)
def test_mdqn_head_edge_cases(case):
    B, A = 33, 4
    fx = _fixture(B, A)
    r = _oracle(B, A, False, case)
    if case == "plain":
        # the clip fixture: in the oracle some rows are clipped and some lie strictly inside (clip, 0)
        assert int((r["tl"] < CLIP).sum()) >= 1 and int(((r["tl"] > CLIP) & (r["tl"] < 0)).sum()) >= 1
        torch.testing.assert_close(r["aux"][:, 0], ALPHA * r["tl"].clamp(CLIP, 0.0), rtol=0, atol=1e-12)
    h = _run_hip(B, A, False, case)
    _compare(h, r)
    ar = torch.arange(B)
    qa = r["q"][ar, fx["act"].long()]
    if case == "terminal":
        torch.testing.assert_close(r["td"], (fx["rew"].double() + r["aux"][:, 0] - qa).abs(), rtol=0, atol=1e-12)
    if case == "equal_q":
        torch.testing.assert_close(r["tl"], torch.full((B,), -TAU * math.log(A), dtype=torch.float64), rtol=0, atol=1e-12)
        torch.testing.assert_close(h["aux"][:, 0], torch.full((B,), -ALPHA * TAU * math.log(A)), rtol=1e-5, atol=0)
    if case == "huge_gaps":
        assert float((r["g1"].topk(2, dim=1).values.diff(dim=1)).abs().min()) > 90.0
        assert torch.equal(r["aux"][:, 1], r["g1"].max(1).values)                # every other exp is 0 in fp64
        torch.testing.assert_close(h["aux"][:, 1], r["g1"].max(1).values.float(), rtol=1e-6, atol=0)
        off = fx["act"].long() != r["g0"].argmax(1)
        assert bool((h["aux"][off, 0] == ALPHA * CLIP).all()) and bool((h["aux"][~off, 0] == 0).all())
    if case == "alpha0":
        assert bool((h["aux"][:, 0] == 0).all())
    if case == "no_isw":
        torch.testing.assert_close(h["dhead"][:, 0].abs(), (r["td"].clamp(max=KAPPA) / B).float(), rtol=1e-4, atol=1e-7)
    # the dueling split of the gradient: the advantage columns sum to zero over the actions
    assert float(h["dhead"][:, 1:].sum(1).abs().max()) <= 4 * 2.0 ** -23 * float(h["dhead"][:, 0].abs().max())


# ------------------------------------------------- 3. side duties, q_out bits
def _ddqn_head_on_same_rows(B, A, isn=None):
    """``ops.head`` (ddqn_head_kernel) with the fixture's online S_t rows, online head and weights: (q_out, the
    region it zeroed)."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    fx = _fixture(B, A)
    dev = lambda t: t.to(DEV)                                            # noqa: E731
    Pon, Ptg = {k: dev(v) for k, v in fx["Pon"].items()}, {k: dev(v) for k, v in fx["Ptg"].items()}
    Hon2 = torch.cat([dev(fx["Hon"]), dev(fx["Htg"][:B])])               # (S_t, some S_t+n rows) of the online net
    td, loss = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    dH, dhead = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16), torch.zeros(B, A + 1, device=DEV)
    q = torch.zeros(B, A, device=DEV)
    flat = torch.full((sum(v.numel() for v in Pon.values()),), 3.0, device=DEV)
    HipBackend().head(Hon2, dev(fx["Htg"][:B]), Pon, Ptg, dev(fx["act"]), dev(fx["rew"]), dev(fx["gam"]),
                      dev(fx["isw"]), True, KAPPA, 1.0 / B, td, loss, dH, dhead, q_out=q, zero=flat, isn=isn)
    torch.cuda.synchronize()
    return q.cpu(), flat.cpu()


def test_side_duties_match_the_ddqn_head():
    """IsNorm outputs and the zeroed head-gradient region as ``ops.head`` leaves them on the same weights;
    q_out is optional."""
    B, A = 33, 4
    fx = _fixture(B, A)
    wscale = torch.full((1,), 1.7, device=DEV)

    def isn():
        return (wscale, torch.full((1,), -1.0, dtype=torch.float64, device=DEV),
                torch.full((1,), 5, dtype=torch.int64, device=DEV))
    isn_m, isn_d = isn(), isn()
    h = _run_hip(B, A, False, "plain", isn=isn_m)
    _, flat = _ddqn_head_on_same_rows(B, A, isn=isn_d)
    assert torch.equal(isn_m[1], isn_d[1]) and float(isn_m[1]) == float(fx["isw"].max().double() / np.float32(1.7))
    assert torch.equal(isn_m[2], isn_d[2]) and int(isn_m[2]) == 5 + int((fx["isw"] > 0).sum())
    assert torch.equal(h["zeroed"], flat) and bool((flat == 0).all())
    h2 = _run_hip(B, A, False, "plain", q_out=False)
    assert torch.equal(h2["td"], h["td"]) and torch.equal(h2["dH"], h["dH"])


@pytest.mark.parametrize("B,A", [(33, 4), (7, 18)])
def test_q_out_bit_equal_to_the_ddqn_head(B, A):
    """q_out against ddqn_head_kernel's on the same S_t rows and online head, bit for bit (both
    instantiations, MAXA = 8 and HEAD_MAXA): both kernels instantiate head_common.h ddqn_head_body with both of
    its forward paths, so wave 0's head_q compiles to the same instructions (docs/PERF_NOTES.md)."""
    h = _run_hip(B, A, False, "plain")
    q, _ = _ddqn_head_on_same_rows(B, A)
    dq = (h["q"].double() - q.double()).abs()
    print(f"q_out vs ddqn_head_kernel ({B}, {A}): {int((dq > 0).sum())} of {dq.numel()} differ, max {float(dq.max()):.3e}")
    assert torch.equal(h["q"], q)


# ----------------------------------------------------------------- 4. sampler
@pytest.mark.parametrize("fused", [False, True])
def test_sampler_obs2(fused):
    """obs2 is bit-equal to obs from tree_sample_kernel and from the optimizer + sample launch; without it
    the same batch is drawn and nothing else is written."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    B, n = 37, 70_001
    be = HipBackend()
    g = torch.Generator().manual_seed(1)
    p0, gr = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV) * 1e-2
    res = {}
    for with_obs2 in (True, False):
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=4)
        fill_replay(rp, 1500, seed=2)
        S = rp.alloc_sample_buffers(B)
        nxt2 = torch.full((B, 4), -7, dtype=torch.int32, device=DEV)
        obs2 = torch.full((B, 4), -7, dtype=torch.int32, device=DEV)
        p, v, m = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        if fused:
            pbf = torch.zeros(n, device=DEV, dtype=torch.bfloat16)
            part, gn = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
            be.optimizer(p, gr, v, m, pbf, 2.5e-4, 0.95, 1.5e-7, 40.0, True, part, gn,
                         sample=(rp, B, S, nxt2, obs2) if with_obs2 else (rp, B, S, nxt2))
        else:
            rp.sample(B, out=S, nxt2=nxt2, **({"obs2": obs2} if with_obs2 else {}))
        torch.cuda.synchronize()
        assert torch.equal(nxt2, S["nxt"]) and torch.equal(S["obs"], rp.obs[S["idx"]])
        assert not torch.equal(S["obs"], S["nxt"])
        assert torch.equal(obs2, S["obs"]) if with_obs2 else bool((obs2 == -7).all())
        res[with_obs2] = (S, p)
    for k in res[True][0]:
        assert torch.equal(res[True][0][k], res[False][0][k]), k
    assert torch.equal(res[True][1], res[False][1])


# -------------------------------------------------------------- 5. whole step
def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"munchausen": True, **rt}})


@pytest.mark.parametrize("dtype,noisy", [("bf16", False), ("fp32", False), ("fp32", True)])
def test_mdqn_learner_step_hip_vs_torch_backend(dtype, noisy):
    """tests/test_gpu_qr.py test_qr_learner_step_hip_vs_torch_backend with the Munchausen target at B = 32,
    with that test's bounds and its clip-norm identity; the row plan on the device."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, noisy=noisy)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.munchausen and L.N == 1 and L.split == split and L.noisy == noisy and L._rows_first == 32
        L.t32.mul_(1.25)                       # a target net that differs from the online net
        from apex_dqn_amd.ops.fused_ops import split_into
        split_into(L.t32, L.tbf, L.tbf_lo)
        L._target_changed()
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        B = L.B
        assert torch.equal(L.slots[2 * B:], L.slots[:B]) and torch.equal(L.slots[B:2 * B], rp.nxt[L.S["idx"]])
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, float(L.gnorm), gn)
        m = L.last_metrics()
        assert m["munchausen_bonus_mean"] <= 0.0 and np.isfinite(m["soft_value_mean"])
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout, L.mdqn_aux.clone())
    assert torch.equal(res["hip"][2], res["torch"][2])
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][5], res["torch"][5], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} HIP step vs the torch backend, noisy {noisy}):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


# ------------------------------------------------------------------ 6. graphs
def test_mdqn_graph_steps_match_eager_steps():
    """steps(4) replaying one 4-update graph == 4 eager step() calls of a twin learner: parameters and
    optimizer state bit-identical (pre-sampling inside the optimizer launch on both)."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res = {}
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        assert L.munchausen and L._presample
        p0 = L.p32.clone()
        if graphs:
            L.steps(4)
            assert L._multi is not None
        else:
            for _ in range(4):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 4 and not torch.equal(p0, L.p32)
        B = L.B
        assert torch.equal(L.slots[2 * B:], L.slots[:B])          # the pre-drawn batch's row plan
        if graphs:
            assert L.graph_matches_eager() is True
        res[graphs] = (L.p32.clone(), L.rms_v.clone(), L.rms_m.clone(), rp.leaf.clone(), L.S["idx"].clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. resume
def test_mdqn_gpu_resume_matches_uninterrupted_run(tmp_path):
    """Save after 3 updates, load into a fresh learner, 3 more: bit-equal to 6 uninterrupted updates."""
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

    def replay():
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=5)
        fill_replay(rp, 1500, seed=2)
        return rp

    cfg = _cfg(32, use_graphs=True, learner={"q_target_sync_freq": 2})
    rp = replay()
    torch.manual_seed(0)
    L = FusedNatureLearner(cfg, DEV, rp)
    for _ in range(3):
        L.step()
    torch.cuda.synchronize()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(3):
        L.step()
    torch.cuda.synchronize()
    rp2 = replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    torch.manual_seed(9)
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.munchausen and L2.num_q_updates == 3
    for _ in range(3):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.S["weights"], L2.S["weights"]), (L.slots, L2.slots)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 8. GPU loop
def test_mdqn_gpu_loop_lock_step():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 20, "q_target_sync_freq": 25},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 20, "use_graphs": True, "munchausen": True,
                                            "env_backend": "fake_ale"}})
    out = train_frames(cfg, DEV, 12, num_envs=16, async_actors=False)
    L, rp = out["learner"], out["replay"]
    torch.cuda.synchronize()
    assert L.munchausen and L.num_q_updates == 12
    live = rp.leaf[rp.leaf != 0]
    assert bool((live > 0).all()) and live.numel() >= 300 and bool(torch.isfinite(live).all())
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
    assert m["munchausen_bonus_mean"] <= 0.0 and np.isfinite(m["soft_value_mean"])
