"""Implicit quantile (IQN) head on the GPU: csrc/iqn_head.hip (``iqn_head_kernel``, csrc/sumtree.hip ``iqn_wgrad_prio_kernel``,
``iqn_actor_head_kernel``) against the fp64 torch oracle (``TorchBackend.iqn_head`` / ``iqn_wgrad`` /
``iqn_actor_head`` on fp64 inputs, tests/iqn_fixtures.py), the tau draws against the host mirror
(learner/iqn.py), bitwise reproducibility across grid sizes and captured graphs, and the fused learner with
the head: the whole step against the torch backend, graphs against eager steps, resume, the GPU loop.

The fixtures, their top-2 gaps and near-kink shares, and the fp32 stand-in's error against the
oracle are checked without a GPU in tests/test_iqn_cpu.py."""
import pytest
import torch

import iqn_fixtures as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(t):
    return None if t is None else t.to(DEV)


def _run_hip(B, A, N, split=False, case="plain", kappa=F.KAPPA, max_blocks=None, isn=False, ctr=F.CTR):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be = HipBackend()
    fx = F.fixture(B, A, split)
    rew, gam, isw = F.case_inputs(fx, case)
    Hon, Htg, Hon_lo, Htg_lo = _dev(fx["Hon"]), _dev(fx["Htg"]), _dev(fx["Hon_lo"]), _dev(fx["Htg_lo"])
    Pon, Ptg = {k: _dev(v) for k, v in fx["Pon"].items()}, {k: _dev(v) for k, v in fx["Ptg"].items()}
    Eon, Etg = {k: _dev(v) for k, v in fx["Eon"].items()}, {k: _dev(v) for k, v in fx["Etg"].items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16)
    dH_lo = torch.zeros_like(dH) if split else None
    dhead = torch.full((B, (A + 1) * N), 7.0, device=DEV)
    q = torch.zeros(B, A, device=DEV)
    taus = torch.full((B, 3, N), -1.0, device=DEV)
    ws = be.iqn_workspace(B, N, DEV)
    shapes = {"wv": (1, 512), "bv": (1,), "wa": (A, 512), "ba": (A,), "wtau": (1024, 64), "btau": (1024,)}
    n = sum(int(torch.tensor(s).prod()) for s in shapes.values())
    flat = torch.full((n,), 3.0, device=DEV)                              # zeroed by the head launch
    gr, o = {}, 0
    for k, s in shapes.items():
        m = int(torch.tensor(s).prod())
        gr[k] = flat[o:o + m].view(s)
        o += m
    isn_out = (torch.full((1,), F.WSCALE, device=DEV), torch.full((1,), -1.0, dtype=torch.float64, device=DEV),
               torch.zeros((), dtype=torch.int64, device=DEV)) if isn else None
    be.iqn_head(Hon, Htg, Pon, Ptg, Eon, Etg, _dev(fx["act"]), _dev(rew), _dev(gam), _dev(isw), N, kappa, 1.0 / B,
                F.seed_q(), torch.tensor([ctr], device=DEV), torch.tensor([F.BASE], device=DEV), td, loss, dH, dhead,
                ws, q_out=q, tau_out=taus, zero=flat, lo=(Hon_lo, Htg_lo, dH_lo) if split else None, isn=isn_out,
                max_blocks=max_blocks)
    torch.cuda.synchronize()
    zeroed = bool((flat == 0).all())
    be.iqn_wgrad(_dev(fx["act"]), ws, gr)
    torch.cuda.synchronize()
    dHj = dH.double() + (dH_lo.double() if split else 0.0)
    return dict(td=td.cpu(), loss=loss.cpu(), dH=dHj.cpu(), dhead=dhead.cpu(), q=q.cpu(), taus=taus.cpu(),
                g={k: v.cpu().clone() for k, v in gr.items()}, zeroed=zeroed,
                isn=None if isn_out is None else float(isn_out[1].cpu()),
                count=None if isn_out is None else int(isn_out[2].cpu()))


# --------------------------------------------------------- 1. kernels vs oracle
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N,max_blocks", [(64, 4, 8, None), (64, 18, 64, None), (64, 6, 21, None),
                                              (64, 2, 2, None), (5, 4, 8, None), (13, 4, 8, 3)])
def test_iqn_head_and_wgrad_kernels_vs_fp64_oracle(B, A, N, max_blocks, split):
    """bf16 single plane and split hi / lo inputs (the oracle works on the joined values).  B = 5: not a
    multiple of the samples per block; (13, 4, 8) with three blocks: a ragged tail and blocks that walk.

    Measured on the CPU (fp64 oracle; tests/test_iqn_cpu.py asserts the bounds used here): the smallest
    top-2 gap of the online next-state q is 2.5e-3 / 1.9e-3 at (64, 4, 8) bf16 / split, 5.1e-1 at
    (64, 18, 64), 2.2e-3 / 2.1e-3 at (64, 6, 21), 3.2e-2 / 3.1e-2 at (64, 2, 2), 7.0e-1 at (5, 4, 8) and
    1.0e-2 / 9.9e-3 at (13, 4, 8): no near-tie at the q tolerance of 1e-4, every sample is compared.  The
    share of the 1024 embedding rows that carry near-kink slack (some |pre| < 1e-5) is 0.6 %, 4.0 %,
    1.6 %, 0.2 %, 0.1 % and 0.2 % in the same order.  The fp32 stand-in (``TorchBackend(torch.float32)``)
    stays within 2.6 % of every tolerance on all twelve problems, so the tolerances of tests/test_gpu_qr.py
    are kept as they are."""
    r = F.oracle(B, A, N, split)
    h = _run_hip(B, A, N, split, max_blocks=max_blocks)
    print(f"B {B} A {A} N {N} split {split}: oracle gap {r['gap']:.3e}, kink share {r['kink_share']:.4f}, errors / tolerance "
          f"{ {k: round(v, 3) for k, v in F.max_errors(h, r).items()} }")
    assert torch.equal(h["taus"], r["taus"])                  # bit-equal to the mirror
    assert h["zeroed"]
    F.compare(h, r)


def test_iqn_head_every_optional_argument_at_once():
    """q_out, tau_out, the zeroed region, the three lo planes, the IS weights and the IS statistic with its
    output and its row count, all given: every member of the argument block the launch passes is read or
    written through, so a member at the wrong offset shows as a wrong number.  Two sample pairs, the second
    with one live row; the smallest head (N = 2).  The statistic is max(isw) / 2 formed in fp64 from the same
    fp32 weights, and the count an integer: both equal the oracle's exactly."""
    B, A, N = 3, 3, 2           # B = DIST_SPB + 1 (csrc/dist_head.h)
    r = F.oracle(B, A, N, True)
    assert r["gap"] >= 1e-3, r["gap"]
    h = _run_hip(B, A, N, True, isn=True)
    assert torch.equal(h["taus"], r["taus"])
    assert h["zeroed"]
    F.compare(h, r)
    assert r["count"] == B and h["count"] == r["count"]
    assert r["isn"] == float(F.fixture(B, A, True)["isw"].max().double() / F.WSCALE) and h["isn"] == r["isn"]


def test_iqn_head_grid_size_does_not_change_a_bit():
    """No float atomics, every sum in a fixed order: one block walking the batch, three blocks and the
    default grid leave the same bits."""
    B, A, N = 13, 4, 8
    ref = _run_hip(B, A, N)
    for mb in (1, 3):
        h = _run_hip(B, A, N, max_blocks=mb)
        for k in ("td", "loss", "dH", "dhead", "q", "taus"):
            assert torch.equal(h[k], ref[k]), (mb, k)
        for k in F.GRADS:
            assert torch.equal(h["g"][k], ref["g"][k]), (mb, k)


# ------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("case", ["rew_hi", "rew_lo", "terminal", "no_isw", "kappa"])
def test_iqn_head_edge_cases(case):
    """All-terminal batches, |u| > kappa everywhere (rew = +-25), weights off, kappa = 0.25."""
    B, A, N = 64, 4, 8
    fx = F.fixture(B, A)
    kappa = 0.25 if case == "kappa" else F.KAPPA
    r = F.oracle(B, A, N, False, case, kappa)
    h = _run_hip(B, A, N, False, case, kappa)
    F.compare(h, r)
    w = torch.ones(B, dtype=torch.float64) if case == "no_isw" else fx["isw"].double()
    tau = r["taus"][:, 0].double()
    if case in ("rew_hi", "rew_lo"):
        # every |u| > kappa, one sign: the gradient is -w gs (tau_i - 1{u < 0}) in the oracle, exactly
        u = (25.0 if case == "rew_hi" else -25.0) + fx["gam"].double()[:, None, None] * r["th_target"][:, None, :] \
            - r["th"][:, :, None]
        assert float(u.abs().min()) > F.KAPPA and bool(((u > 0) == (case == "rew_hi")).all())
        g_ref = -w[:, None] * (1.0 / B) * (tau - (0.0 if case == "rew_hi" else 1.0))
        torch.testing.assert_close(r["dhead"][:, :N], g_ref, rtol=1e-12, atol=1e-18)
        torch.testing.assert_close(h["dhead"][:, :N], g_ref.float(), rtol=1e-4, atol=1e-7)
    if case == "terminal":
        qa = r["q"][torch.arange(B), fx["act"].long()]
        torch.testing.assert_close(h["td"], (fx["rew"].double() - qa).abs().float(), rtol=1e-4, atol=1e-4)
    dadv = h["dhead"][:, N:].reshape(B, A, N)
    assert float(dadv.sum(1).abs().max()) <= 4 * 2.0 ** -23 * float(h["dhead"][:, :N].abs().max())


# ------------------------------------------- 3. IsNorm and the zeroed region
def test_iqn_head_is_norm_and_zeroed_region_match_qr_head():
    """The batch-max IS statistic and the zeroed head-gradient region are dist_head_side's: the same
    numbers ``ops.qr_head`` leaves for the same weights."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    B, A, N = 64, 4, 8
    h = _run_hip(B, A, N, isn=True)
    assert h["zeroed"]
    be = HipBackend()
    fx = F.fixture(B, A)
    g = torch.Generator().manual_seed(5)
    P = {"wv": torch.randn(N, 512, generator=g) * 0.05, "bv": torch.randn(N, generator=g),
         "wa": torch.randn(A * N, 512, generator=g) * 0.05, "ba": torch.randn(A * N, generator=g)}
    P = {k: v.to(DEV) for k, v in P.items()}
    flat = torch.full((1000,), 3.0, device=DEV)
    out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    td, loss = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    be.qr_head(_dev(fx["Hon"]), _dev(fx["Htg"]), P, P, _dev(fx["act"]), _dev(fx["rew"]), _dev(fx["gam"]), _dev(fx["isw"]),
               N, 1.0, 1.0 / B, td, loss, torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16),
               torch.zeros(B, (A + 1) * N, device=DEV), zero=flat, isn=(torch.full((1,), 2.0, device=DEV), out))
    torch.cuda.synchronize()
    assert bool((flat == 0).all())
    assert h["isn"] == float(out.cpu()) and h["isn"] == float(fx["isw"].max().double() / 2.0)


# -------------------------------------------------------------- 4. actor head
@pytest.mark.parametrize("midpoint", [False, True])
@pytest.mark.parametrize("K", [1, 32, 64])
@pytest.mark.parametrize("E", [5, 64])
def test_iqn_actor_head_vs_oracle(E, K, midpoint):
    """q to the QR actor head's tolerance (1e-4); the greedy action wherever the oracle's top-2 gap exceeds
    it; the drawn fractions bit-equal to the mirror; with eps = 1 the actions of the scalar actor
    head (the same counter-RNG words)."""
    from apex_dqn_amd.learner.iqn import midpoint_taus, stream_taus
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend
    A, stream, t = 6, 5, 11
    fx = F.fixture(64, A)
    H, P, Em = fx["Hon"][:E].contiguous(), fx["Pon"], fx["Eon"]
    q_ref, a_ref = torch.zeros(E, A, dtype=torch.float64), torch.zeros(E, dtype=torch.int32)
    tau_ref = torch.zeros(E, K)
    eps, ctr, tctr = torch.zeros(E), torch.zeros(1, dtype=torch.int64), torch.tensor([t])
    TorchBackend(torch.float64).iqn_actor_head(H.double(), {k: v.double() for k, v in P.items()},
                                               {k: v.double() for k, v in Em.items()}, eps, ctr, 5, F.seed_q(), tctr,
                                               stream, K, midpoint, q_ref, a_ref, tau_out=tau_ref)
    want = midpoint_taus(K)[None, :].expand(E, K) if midpoint else stream_taus(F.seed_q(), 64 * t + stream, E, K)
    assert torch.equal(tau_ref, want)
    be = HipBackend()
    Pd, Ed = {k: v.to(DEV) for k, v in P.items()}, {k: v.to(DEV) for k, v in Em.items()}
    q, a = torch.zeros(E, A, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV)
    taus = torch.full((E, K), -1.0, device=DEV)
    be.iqn_actor_head(H.to(DEV), Pd, Ed, eps.to(DEV), ctr.to(DEV), 5, F.seed_q(), tctr.to(DEV), stream, K, midpoint, q, a,
                      tau_out=taus)
    torch.cuda.synchronize()
    assert torch.equal(taus.cpu(), want)
    err = float((q.cpu().double() - q_ref).abs().max())
    top = q_ref.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4
    print(f"E {E} K {K} midpoint {midpoint}: q err {err:.2e}, clear rows {int(clear.sum())} / {E}")
    assert err < 1e-4
    assert int(clear.sum()) >= E - 1
    assert torch.equal(a.cpu()[clear], q_ref.argmax(1).to(torch.int32)[clear])
    one = torch.ones(E, device=DEV)
    a1, a2 = torch.zeros_like(a), torch.zeros_like(a)
    c3 = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    be.iqn_actor_head(H.to(DEV), Pd, Ed, one, c3, 9, F.seed_q(), tctr.to(DEV), stream, K, midpoint, q, a1)
    Ps = {"wv": Pd["wv"].reshape(512).contiguous(), "bv": Pd["bv"], "wa": Pd["wa"], "ba": Pd["ba"]}
    be.actor_head(H.to(DEV), Ps, one, c3, 9, torch.zeros(E, A, device=DEV), a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and len(set(a1.tolist())) > 1


# ------------------------------------------------------------------ 5. graphs
def test_iqn_graph_replays_draw_fresh_taus_and_match_eager_launches():
    """A captured head + weight-gradient launch replayed four times, the draw counter advanced on the
    device between replays, leaves the bits of four eager launches: the update index is read on the
    device, so every replay draws fresh fractions with no host round trip."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    B, A, N = 16, 4, 8
    be = HipBackend()
    fx = F.fixture(64, A)
    Hon = torch.cat([fx["Hon"][:B], fx["Hon"][64:64 + B]]).to(DEV)
    Htg = fx["Htg"][:B].contiguous().to(DEV)
    Pon, Ptg = {k: _dev(v) for k, v in fx["Pon"].items()}, {k: _dev(v) for k, v in fx["Ptg"].items()}
    Eon, Etg = {k: _dev(v) for k, v in fx["Eon"].items()}, {k: _dev(v) for k, v in fx["Etg"].items()}
    act, rew, gam, isw = (_dev(fx[k][:B].contiguous()) for k in ("act", "rew", "gam", "isw"))
    ctr, base = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    td, loss = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    dH, dhead = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16), torch.zeros(B, (A + 1) * N, device=DEV)
    taus = torch.zeros(B, 3, N, device=DEV)
    ws = be.iqn_workspace(B, N, DEV)
    gr = {"wv": torch.zeros(1, 512, device=DEV), "bv": torch.zeros(1, device=DEV), "wa": torch.zeros(A, 512, device=DEV),
          "ba": torch.zeros(A, device=DEV), "wtau": torch.zeros(1024, 64, device=DEV), "btau": torch.zeros(1024, device=DEV)}

    def launch():
        be.iqn_head(Hon, Htg, Pon, Ptg, Eon, Etg, act, rew, gam, isw, N, 1.0, 1.0 / B, F.seed_q(), ctr, base, td, loss,
                    dH, dhead, ws, tau_out=taus)
        be.iqn_wgrad(act, ws, gr)
        ctr.add_(1)

    def snap():
        return [t.clone() for t in (taus, td, loss, dH, dhead, *gr.values())]

    eager = []
    for _ in range(4):
        launch()
        eager.append(snap())
    torch.cuda.synchronize()
    ctr.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()                       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    ctr.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    ctr.zero_()
    replayed = []
    for _ in range(4):
        graph.replay()
        replayed.append(snap())
    torch.cuda.synchronize()
    assert int(ctr.item()) == 4
    for u in range(4):
        for x, y in zip(eager[u], replayed[u]):
            assert torch.equal(x, y), u
    draws = {tuple(e[0].flatten().tolist()) for e in eager}
    assert len(draws) == 4
    from apex_dqn_amd.learner.iqn import learner_taus
    assert torch.equal(replayed[3][0].cpu(), learner_taus(F.seed_q(), 3, B, N))


# ------------------------------------------------------- 6. the learner's step
def _fill_replay(rp, K, A=6, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    seqs = rp.append_frames(rng.integers(0, 255, (K + 8, 84, 84), dtype=np.uint8))
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, A, K), R=rng.normal(size=K).astype(np.float32),
                   Gamma=np.where(rng.random(K) < 0.1, 0.0, 0.97).astype(np.float32),
                   priority=rng.random(K).astype(np.float32) * 3 + 0.01))


def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"num_atoms": 8, "dist_head": "implicit", **rt}})


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_iqn_learner_step_hip_vs_torch_backend(dtype):
    """tests/test_gpu_qr.py test_qr_learner_step_hip_vs_torch_backend with the implicit head (8 samples) at
    B = 32, in the bf16-operand mode and the fp32 (split) mode, with that test's bounds and its clip-norm
    identity; both backends draw the same fractions."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.iqn import iqn_seed, learner_taus
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        _fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.N == 8 and L.implicit and L.split == split
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, float(L.gnorm), gn)
        assert torch.equal(L.tau_out.cpu(), learner_taus(iqn_seed(cfg.Runtime.seed), 0, 32, 8))
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout)
    assert torch.equal(res["hip"][2], res["torch"][2])
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} HIP step vs the torch backend):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0 and float(gt["wtau"].norm()) > 0


def test_iqn_graph_steps_match_eager_steps():
    """steps(4) replaying one 4-update graph == 4 eager step() calls of a twin learner, bit for bit
    (parameters, optimizer state, priorities, the next batch), each update with its own fractions."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.iqn import iqn_seed, learner_taus
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res, draws = {}, []
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        _fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        assert L.implicit and L._presample
        p0 = L.p32.clone()
        if graphs:
            L.steps(4)
            assert L._multi is not None
        else:
            for _ in range(4):
                L.step()
                draws.append(L.tau_out.clone())
        torch.cuda.synchronize()
        assert L.num_q_updates == 4 and L.update_index() == 4 and not torch.equal(p0, L.p32)
        taus = L.tau_out.clone()       # (graph_matches_eager below runs further updates and restores the state,
        assert torch.equal(taus.cpu(), learner_taus(iqn_seed(cfg.Runtime.seed), 3, 64, 8))     # not this output)
        if graphs:
            assert L.graph_matches_eager() is True
        res[graphs] = (L.p32.clone(), L.rms_v.clone(), L.rms_m.clone(), rp.leaf.clone(), L.S["idx"].clone(), taus)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert len({tuple(t.flatten().tolist()) for t in draws}) == 4


def test_iqn_gpu_resume_matches_uninterrupted_run(tmp_path):
    """Save after 3 updates, load into a fresh learner, 3 more: bit-equal to 6 uninterrupted updates."""
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

    def replay():
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=5)
        _fill_replay(rp, 1500, seed=2)
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
    assert L2.implicit and L2.num_q_updates == 3
    for _ in range(3):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.S["weights"], L2.S["weights"]), (L.slots, L2.slots), (L.tau_out, L2.tau_out)):
        assert torch.equal(a, b)


def test_iqn_gpu_loop_lock_step():
    import numpy as np
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 20, "q_target_sync_freq": 25},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 20, "use_graphs": True, "num_atoms": 8,
                                            "dist_head": "implicit", "env_backend": "fake_ale"}})
    out = train_frames(cfg, DEV, 12, num_envs=16, async_actors=False)
    L, rp = out["learner"], out["replay"]
    torch.cuda.synchronize()
    assert L.implicit and L.num_q_updates == 12
    live = rp.leaf[rp.leaf != 0]
    assert bool((live > 0).all()) and live.numel() >= 300 and bool(torch.isfinite(live).all())
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
    q = out["actors"].q
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all()) and float(q.abs().max()) > 0


def test_iqn_wgrad_with_the_priority_write_back_in_the_same_launch():
    """``iqn_wgrad`` with ``prio``: block 0 of the launch writes the priorities back (as ``head_wgrad_prio_kernel``
    does for the other heads).  The gradients are the bits of the launch without it, and the tree is what a separate ``update_priorities`` leaves on a twin replay."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    B, A, N = 64, 4, 8
    ref = _run_hip(B, A, N)
    be = HipBackend()
    fx = F.fixture(B, A)
    rps = []
    for _ in range(2):
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        _fill_replay(rp, 1500, seed=11)
        rps.append(rp)
    g = torch.Generator().manual_seed(4)
    idx = torch.randint(0, 1500, (B,), generator=g).to(DEV)
    idx[5] = idx[40]                                            # a duplicated leaf: the later write wins
    td = (torch.rand(B, generator=g) * 2).to(DEV)
    gen = rps[0].gen[idx].clone()
    # the head launch again, into a workspace of this test's own
    Pon, Ptg = {k: _dev(v) for k, v in fx["Pon"].items()}, {k: _dev(v) for k, v in fx["Ptg"].items()}
    Eon, Etg = {k: _dev(v) for k, v in fx["Eon"].items()}, {k: _dev(v) for k, v in fx["Etg"].items()}
    ws = be.iqn_workspace(B, N, DEV)
    be.iqn_head(_dev(fx["Hon"]), _dev(fx["Htg"]), Pon, Ptg, Eon, Etg, _dev(fx["act"]), _dev(fx["rew"]), _dev(fx["gam"]),
                _dev(fx["isw"]), N, F.KAPPA, 1.0 / B, F.seed_q(), torch.tensor([F.CTR], device=DEV),
                torch.tensor([F.BASE], device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, device=DEV),
                torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16), torch.zeros(B, (A + 1) * N, device=DEV), ws)
    z = lambda *s: torch.full(s, 3.0, device=DEV)                        # noqa: E731
    for rep in range(2):
        gr = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
        c0 = int(rps[0].ctr.item())
        be.iqn_wgrad(_dev(fx["act"]), ws, gr, prio=(rps[0], idx, gen, td) if rep == 0 else None)
        torch.cuda.synchronize()
        for k in F.GRADS:
            assert torch.equal(gr[k].cpu(), ref["g"][k]), (rep, k)
        if rep == 0:
            assert int(rps[0].ctr.item()) == c0 + 1
    rps[1].update_priorities(idx, td, gen)
    torch.cuda.synchronize()
    assert torch.equal(rps[0].leaf, rps[1].leaf) and not torch.equal(rps[0].leaf[idx], torch.zeros_like(td))
    assert torch.equal(rps[0].ctr, rps[1].ctr)
    torch.testing.assert_close(rps[0].nodes, rps[1].nodes, rtol=1e-12, atol=1e-9)
