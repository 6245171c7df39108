"""The soft (Polyak) target network, ``Runtime.target_ema_rate``, on the GPU: the optimizer kernels'
EMA instantiations (csrc/rmsprop_common.h) in every launch form against the host mirror
(learner/schedules.py ``target_ema``), the target set's fragment stores, and the learner with it:
rate 1 against a hard sync, replayed graphs, the whole step against the torch backend, a resume and
the GPU loop."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.learner import schedules as sch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RHO = 0.25
ADAM = dict(lr=2.5e-4, warmup=2, decay=3, lr_end=2.5e-5, b1=0.9, b2=0.999, eps=1.5e-4, clip=40.0)


def _replay(seed=7, C=4):
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    rp = GpuReplayShard(2000, 2000, 2100, C, device=DEV, seed=seed)
    rng = np.random.default_rng(11)
    K = 1500
    seqs = rp.append_frames(rng.integers(0, 255, (K + 8, 84, 84), dtype=np.uint8))
    st = np.stack([seqs[i:i + C] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, 6, K), R=rng.normal(size=K).astype(np.float32),
                   Gamma=np.where(rng.random(K) < 0.1, 0.0, 0.97).astype(np.float32),
                   priority=rng.random(K).astype(np.float32) * 3 + 0.01))
    return rp


def _cfg(rt, B=64, C=4, **learner):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": {"state_shape": [C, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner}, "Runtime": dict(rt)})


def _learner(rt, B=64, C=4, backend="hip", rp=None, seed=0, **learner):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(seed)
    return FusedNatureLearner(_cfg(rt, B, C, **learner), DEV, rp if rp is not None else _replay(C=C), backend=backend)


def _split(t32, split):
    """The project's bf16 planes of an fp32 tensor: hi = bf16(t), lo = bf16(t - hi)."""
    hi = t32.to(torch.bfloat16)
    return hi, ((t32 - hi.float()).to(torch.bfloat16) if split else None)


# ------------------------------------------------------------------ 1. kernel
def _spec(mode, ctr=None):
    if mode == "rmsprop":
        return None
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV) if ctr is None else ctr
    base = torch.zeros(1, dtype=torch.int64, device=DEV)
    kind = "adam" if mode == "adam" else "rmsprop"
    return sch.OptSpec(kind, ctr, base, ADAM["lr"], ADAM["warmup"], ADAM["decay"], ADAM["lr_end"], ADAM["b1"],
                       ADAM["b2"], ADAM["eps"])


@pytest.fixture(scope="module")
def problem():
    """n = 1,048,583 (tests/test_gpu_opt_schedules.py's size): not a multiple of 4 and two sweeps of the
    fused launch's 256 x 512 threads, so its peeled first chunk, steady loop and scalar tail all run."""
    n = 1_048_583
    g = torch.Generator(device="cpu").manual_seed(2)
    p0, t0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (0.01, 0.5)]      # (the second one engages the clip)
    return p0.to(DEV), t0.to(DEV), [x.to(DEV) for x in grads]


def _run_kernel(p0, t0, grads, mode, split, form, with_target, rp=None, B=64):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    n = p0.numel()
    be = HipBackend()
    spec = _spec(mode, rp.ctr if rp is not None else None)
    ctr = spec.ctr if spec is not None else (rp.ctr if rp is not None else None)
    p, v, m = p0.clone(), torch.full((n,), 1e-6, device=DEV), torch.full((n,), 1e-4, device=DEV)
    hi = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    lo = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if split else None
    t = t0.clone()
    th = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    tl = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if split else None
    part, gn = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    S = nxt2 = None
    if rp is not None:
        S, nxt2 = rp.alloc_sample_buffers(B), torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    trail = []
    for gr in grads:
        if ctr is not None:
            ctr += 1
        kw = dict(pb_lo=lo, **({"opt": spec} if spec is not None else {}),
                  **({"target": (t, th, tl, RHO, None)} if with_target else {}))
        t_before = t.clone()
        if form == "plain":
            be.optimizer(p, gr, v, m, hi, ADAM["lr"], 0.95, 1.5e-7, ADAM["clip"], True, part, gn, **kw)
        else:
            npart = be.grad_sqnorm_partials(gr, part)
            if form == "fused":
                kw["sample"] = (rp, B, S, nxt2)
            be.optimizer(p, gr, v, m, hi, ADAM["lr"], 0.95, 1.5e-7, ADAM["clip"], True, part, gn,
                         norm_total=(part, npart), **kw)
        if rp is not None and form != "fused":
            rp.sample(B, out=S, nxt2=nxt2)
        torch.cuda.synchronize()
        trail.append((t_before, p.clone(), t.clone()))
    return dict(p=p, v=v, m=m, hi=hi, lo=lo, t=t, th=th, tl=tl, gn=gn, S=S, nxt2=nxt2, trail=trail)


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("mode", ["rmsprop", "rmsprop_sched", "adam"])
def test_ema_kernel_against_the_mirror(problem, mode, split):
    """Two updates at n = 1,048,583 in the plain launch (256-thread blocks) and the fused optimizer + sample
    launch (512-thread blocks, two sweeps): the online outputs are the bits of the same call without a
    target, t is the mirror applied on the host to the GPU's own p', tb / tb_lo are the split of t."""
    p0, t0, grads = problem
    for form in ("plain", "fused"):
        rps = [_replay(seed=4), _replay(seed=4)] if form == "fused" else [None, None]
        base = _run_kernel(p0, t0, grads, mode, split, form, False, rp=rps[0])
        ema = _run_kernel(p0, t0, grads, mode, split, form, True, rp=rps[1])
        for k in ("p", "v", "m", "hi", "gn") + (("lo",) if split else ()):
            assert torch.equal(base[k], ema[k]), (form, k)
        assert torch.equal(base["t"], t0) and not base["th"].any()          # no target: untouched
        for u, (tb, pn, tn) in enumerate(ema["trail"]):
            want = sch.target_ema(tb.cpu().numpy(), pn.cpu().numpy(), RHO)
            got = tn.cpu().numpy()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (form, u, bad[:8], got[bad[:8]], want[bad[:8]])
        hi, lo = _split(ema["t"], split)
        assert torch.equal(ema["th"].view(torch.int16), hi.view(torch.int16))
        if split:
            assert torch.equal(ema["tl"].view(torch.int16), lo.view(torch.int16))
        if form == "fused":
            for k in base["S"]:
                assert torch.equal(base["S"][k], ema["S"][k]), k


@pytest.mark.parametrize("mode", ["rmsprop", "adam"])
def test_ema_launch_forms_bit_identical(mode):
    """Plain, producer-partials and fused-with-the-sample launches at n = 100,003 leave identical bits in
    every output, the target's included, and the fused form draws the batch a sample launch draws."""
    n = 100_003
    g = torch.Generator(device="cpu").manual_seed(1)
    p0, t0 = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    grads = [(torch.randn(n, generator=g) * 1e-2).to(DEV) for _ in range(2)]
    res = {f: _run_kernel(p0, t0, grads, mode, True, f, True, rp=_replay(seed=4)) for f in ("plain", "partials", "fused")}
    a = res["plain"]
    assert np.array_equal(a["t"].cpu().numpy(), sch.target_ema(a["trail"][1][0].cpu().numpy(), a["p"].cpu().numpy(), RHO))
    for f in ("partials", "fused"):
        b = res[f]
        for k in ("p", "v", "m", "hi", "lo", "t", "th", "tl", "gn", "nxt2"):
            assert torch.equal(a[k].view(torch.int16) if a[k].dtype == torch.bfloat16 else a[k],
                               b[k].view(torch.int16) if b[k].dtype == torch.bfloat16 else b[k]), (f, k)
        for k in a["S"]:
            assert torch.equal(a["S"][k], b["S"][k]), (f, k)


def test_sharded_launch_and_bad_target_blocks_are_refused():
    from apex_dqn_amd.ops.fused_ops import HipBackend
    n = 8192
    be, rp = HipBackend(), _replay(seed=4)
    z = lambda dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    p, g, v, m, t = z(), z(), z(), z(), z()
    hi, th, tl = z(torch.bfloat16), z(torch.bfloat16), z(torch.bfloat16)
    part, gn = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    S, nxt2 = rp.alloc_sample_buffers(8), torch.zeros(8, 4, dtype=torch.int32, device=DEV)
    args = (p, g, v, m, hi, 1e-4, 0.95, 1.5e-7, 40.0, True, part, gn)
    with pytest.raises(ValueError):           # the sharded (SEG) form takes no target
        be.optimizer(*args, norm_total=(part, 1), sample=(rp, 8, S, nxt2), segs=[(0, 4096)], target=(t, th, None, RHO, None))
    with pytest.raises(RuntimeError):         # a rate outside [0, 1]: the launcher refuses, nothing runs
        be.optimizer(*args, target=(t, th, None, 1.5, None))
    with pytest.raises(RuntimeError):         # misaligned target (the float4 path)
        be.optimizer(*args, target=(torch.zeros(n + 1, device=DEV)[1:], th, None, RHO, None))
    torch.cuda.synchronize()
    assert not t.any() and not th.any()


# ------------------------------------------------------------ 2. fragments
def _frag_buffers(L):
    from apex_dqn_amd.ops import conv as C
    ws = L.ops.ws
    return [ws.get(("cf_w1frag",), C.CF_W1FRAG_BYTES, DEV, torch.uint8),
            ws.get(("cf_c2f_wfrag",), 4 * 8192 * 16, DEV, torch.uint8),
            ws.get(("cf_c3f",), C.C3F_BYTES, DEV, torch.uint8)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 4])
def test_target_fragments_equal_fresh_pack(C, dtype):
    """tests/test_gpu_opt_schedules.py test_adam_frag_out_equals_fresh_pack for the other set: after real
    updates the target halves of the conv1 / C2F / C3F buffers equal a fresh pack of the learner's target
    weights byte for byte, and the online halves a fresh pack of the online weights (untouched by it)."""
    L = _learner({"use_graphs": False, "dtype": dtype, "target_ema_rate": RHO}, C=C)
    assert L._frag_out is not None and L._frag_out_t is not None and L._tgt_current()
    n1 = 1024 * C * 16
    first = [b.clone() for b in _frag_buffers(L)]
    for _ in range(3):
        L.step()
    torch.cuda.synchronize()
    assert not torch.equal(L.t32, L.p32)
    bufs = _frag_buffers(L)
    got = [b.clone() for b in bufs]
    half = [n1, 2 * 8192 * 16, 2 * 4608 * 16]
    for name, g, f, h in zip(("conv1", "conv2", "conv3"), got, first, half):
        assert not torch.equal(g[h:2 * h], f[h:2 * h]), f"{name}: the target half never changed"
    c1, c2 = L._conv12_weights()
    L.ops.conv12_pack(c1, c2, L.rt.obs_scale, sets=2, c3=L._conv3_weights())
    torch.cuda.synchronize()
    for name, g, b, h in zip(("conv1", "conv2", "conv3"), got, bufs, half):
        assert torch.equal(g[h:2 * h], b[h:2 * h]), f"{name} target fragments differ from the pack launch"
        assert torch.equal(g, b), f"{name}: the pack of the target set changed other bytes"
    L.ops.conv12_pack(c1, c2, L.rt.obs_scale, sets=1, c3=L._conv3_weights())
    torch.cuda.synchronize()
    for name, g, b in zip(("conv1", "conv2", "conv3"), got, bufs):
        assert torch.equal(g, b), f"{name} online fragments differ from the pack launch"


# ------------------------------------------------------- 3. rate 1 = hard sync
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rate_one_equals_hard_sync_every_update(dtype):
    A = _learner({"use_graphs": False, "dtype": dtype, "target_ema_rate": 1.0}, q_target_sync_freq=1000)
    B = _learner({"use_graphs": False, "dtype": dtype}, q_target_sync_freq=1)
    for u in range(3):
        A.step()
        B.step()
        torch.cuda.synchronize()
        for name in ("p32", "rms_v", "rms_m", "t32", "_tbf_all", "td_abs"):
            assert torch.equal(getattr(A, name), getattr(B, name)), (u, name)     # (by value: -0 == +0)
    assert torch.equal(A.t32, A.p32)


# ------------------------------------------------------------------ 4. graphs
class _Counting:
    def __init__(self, graph):
        self.graph, self.n = graph, 0

    def replay(self):
        self.n += 1
        return self.graph.replay()


def _state(L):
    return [t.clone() for t in (L.p32, L.t32, L._pbf_all, L._tbf_all, L.rms_v, L.rms_m)] + \
        [b.clone() for b in _frag_buffers(L)]


def test_graphs_do_not_break_at_sync_boundaries_and_equal_eager():
    """graph_steps = 4, q_target_sync_freq = 3, steps(8): two replays of the 4-update graph and no single
    step (the hard sync would force 3 + 1 + ...); the result is 8 eager step() calls bit for bit."""
    rt = {"dtype": "fp32", "graph_steps": 4, "target_ema_rate": RHO}
    G = _learner({**rt, "use_graphs": True}, q_target_sync_freq=3)
    G.prepare_graphs(multi=True)
    multi, single = _Counting(G._multi), _Counting(G._graphs)
    G._multi, G._graphs = multi, single
    G.steps(8)
    torch.cuda.synchronize()
    assert (multi.n, single.n) == (2, 0) and G.num_q_updates == G.update_index() == 8
    G._multi, G._graphs = multi.graph, single.graph
    E = _learner({**rt, "use_graphs": False}, q_target_sync_freq=3)
    for _ in range(8):
        E.step()
    torch.cuda.synchronize()
    names = ("p32", "t32", "_pbf_all", "_tbf_all", "rms_v", "rms_m", "conv1 frags", "conv2 frags", "conv3 frags")
    for name, a, b in zip(names, _state(G), _state(E)):
        assert torch.equal(a, b), name
    assert not torch.equal(G.t32, G.p32)
    before = _state(G)
    assert G.graph_matches_eager() is True
    torch.cuda.synchronize()
    for name, a, b in zip(names, before, _state(G)):
        assert torch.equal(a, b), f"graph_matches_eager changed {name}"


# -------------------------------------------------------------- 5. whole step
HEADS = {
    "scalar_fp32": ({"dtype": "fp32"}, True),
    "scalar_bf16": ({"dtype": "bf16"}, True),
    "c51_noisy": ({"dtype": "fp32", "num_atoms": 51, "noisy": True}, True),
    "iqn": ({"dtype": "fp32", "num_atoms": 8, "dist_head": "implicit"}, True),
    "munchausen": ({"dtype": "fp32", "munchausen": True}, True),
    "no_presample": ({"dtype": "fp32"}, False),       # the forward repacks the target set every update
}


def _step_bounds(case, u, H, T):
    """The existing whole-step tests' checks on one update taken by both backends from one state."""
    for L, be in ((H, "hip"), (T, "torch")):
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, u, float(L.gnorm), gn)
    torch.testing.assert_close(H.td_abs, T.td_abs, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(H.loss_b, T.loss_b, rtol=5e-2, atol=5e-2)
    gh, gt = H.layout.views(H.g32), T.layout.views(T.g32)
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({case}, update {u + 1}, HIP step vs the torch backend):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


@pytest.mark.parametrize("case", list(HEADS))
def test_two_updates_hip_vs_torch_backend(case):
    """Two updates of the HIP step against the torch backend at B = 32, each with the bounds of the existing
    whole-step tests of these heads (tests/test_gpu_qr.py test_qr_learner_step_hip_vs_torch_backend: 5e-2 on
    td_abs and loss_b, 0.2 on the per-segment gradient error, the clip-norm identity), from a target that
    differs from the online net, so update 2 reads a target that is neither net of update 1.  Each backend's
    t32 is the mirror of its own p32 after both updates, bit for bit, and its planes the split of it.

    The bounds are those of ONE step taken by both backends from one state, so the torch learner starts
    update 2 from the HIP learner's state after update 1 (parameters, optimizer state, the averaged target in
    t32 / planes, the replay tree); the HIP learner reads the target in the formats its own optimizer launch
    wrote.  Two free-running learners are not comparable at these bounds in bf16, with or without the soft
    target: centered RMSprop's first update moves every weight by lr / sqrt(0.0475) = 2.9e-4 in the direction
    of its gradient's sign, the bf16 step's gradients differ from the torch backend's by up to 9 % per segment
    at update 1 (bound 0.2), so small gradients change sign and the parameters part by up to 1.1e-3; measured
    at update 2, free-running: 0.275 (rho = 0.25) and 0.265 (rho = 0, the hard-sync path) on the worst
    segment, against 0.093 from one state; fp32: 2e-4 either way."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.ops.fused_ops import split_into
    rt, presample = HEADS[case]
    split = rt["dtype"] == "fp32"
    Ls = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        cfg = _cfg({**rt, "use_graphs": False, "presample": presample, "target_ema_rate": RHO}, B=32,
                   q_target_sync_freq=1)
        L = FusedNatureLearner(cfg, DEV, _replay(), backend=be, split=split)
        assert L.ema == RHO and L.split == split
        assert (L._frag_out_t is not None) == (be == "hip" and presample)
        L.t32.mul_(1.25)
        split_into(L.t32, L.tbf, L.tbf_lo)
        L._target_changed()
        if be == "torch":
            L.ops.dtype = torch.float32
        Ls[be] = L
    H, T = Ls["hip"], Ls["torch"]
    for u in range(2):
        if u == 1:
            for name in ("p32", "_pbf_all", "rms_v", "rms_m", "t32", "_tbf_all"):
                getattr(T, name).copy_(getattr(H, name))
            for name in ("leaf", "nodes", "min_bits"):
                getattr(T.replay, name).copy_(getattr(H.replay, name))
            T._online_changed()
            T._target_changed()
        # the update's batch, drawn at its head on both (the draw the pre-sample made: same counter)
        H._sample()
        T._sample()
        assert torch.equal(H.S["idx"], T.S["idx"]), u
        t0 = {be: L.t32.cpu().numpy() for be, L in Ls.items()}
        H.step()
        T.step()
        torch.cuda.synchronize()
        if u == 1:
            assert not torch.equal(H.t32, H.p32)
        for be, L in Ls.items():
            assert np.array_equal(L.t32.cpu().numpy(), sch.target_ema(t0[be], L.p32.cpu().numpy(), RHO)), (be, u)
            hi, lo = _split(L.t32, split)
            assert torch.equal(L.tbf.float(), hi.float()) and (not split or torch.equal(L.tbf_lo.float(), lo.float()))
        _step_bounds(case, u, H, T)


# ------------------------------------------------------------------ 6. resume
def test_gpu_resume_matches_uninterrupted_run(tmp_path):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg = _cfg({"use_graphs": True, "graph_steps": 4, "target_ema_rate": RHO, "noisy": True}, q_target_sync_freq=3)
    rp = _replay(seed=5)
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
    rp2 = _replay(seed=5)
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.num_q_updates == L2.update_index() == 3 and not torch.equal(L2.t32, L2.p32)
    for _ in range(3):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32),
                 (L._tbf_all, L2._tbf_all), (rp.leaf, rp2.leaf), (rp.ctr, rp2.ctr), (L.td_abs, L2.td_abs)):
        assert torch.equal(a, b)
    assert L.last_metrics()["target_gap"] == L2.last_metrics()["target_gap"] > 0


# ---------------------------------------------------------------- 7. GPU loop
def test_gpu_loop_lock_step_on_fake_ale():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "PongNoFrameskip-v4"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 8, "q_target_sync_freq": 5},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 8, "use_graphs": True, "graph_steps": 4,
                                            "env_backend": "fake_ale", "target_ema_rate": RHO}})
    out = train_frames(cfg, DEV, 16, num_envs=16, async_actors=False)
    L = out["learner"]
    torch.cuda.synchronize()
    assert L.ema == RHO and L.num_q_updates == L.update_index() == 16
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0 and 0 < m["target_gap"] < 1
    # 16 updates without one hard sync: the target trails the online net, and its planes are its split
    assert not torch.equal(L.t32, L.p32)
    hi, lo = _split(L.t32, L.split)
    assert torch.equal(L.tbf.float(), hi.float()) and torch.equal(L.tbf_lo.float(), lo.float())
