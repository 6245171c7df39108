"""Periodic shrink-and-perturb resets, ``Runtime.reset_interval``, on the GPU: ``reset_perturb_kernel``
(csrc/reset.hip) against the host mirror (learner/reset.py ``apply_reset``) bit for bit, the launcher's refusals,
the fragment buffers after ``reset_now``, and the learner with it: the whole step against the torch backend,
replayed graphs that break at the boundaries and read Adam's reset word, a resume and the GPU loop."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.learner import reset as RS
from apex_dqn_amd.learner import schedules as sch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
f32 = np.float32
ADAM = {"optimizer": "adam", "lr": 2.5e-4, "lr_warmup_steps": 2}


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


def _cfg(rt, B=64, C=4, A=6, **learner):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": {"state_shape": [C, 84, 84], "action_dim": A, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner}, "Runtime": dict(rt)})


def _learner(rt, B=64, C=4, backend="hip", rp=None, seed=0, **learner):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(seed)
    return FusedNatureLearner(_cfg(rt, B, C, **learner), DEV, rp if rp is not None else _replay(C=C), backend=backend)


def _split(t32, split):
    """The project's bf16 planes of an fp32 tensor: hi = bf16(t), lo = bf16(t - hi)."""
    hi = t32.to(torch.bfloat16)
    return hi, ((t32 - hi.float()).to(torch.bfloat16) if split else None)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ------------------------------------------------------------------ 1. kernel
LAYOUTS = {
    "c1_a2_scalar": (dict(), dict(C=1, A=2)),
    "nature32": (dict(network="nature32"), dict(C=4, A=4)),
    "noisy3": (dict(noisy=True, num_atoms=3), dict(C=4, A=3, num_atoms=3, noisy=True)),
    "implicit": (dict(num_atoms=8, dist_head="implicit"), dict(C=4, A=4, implicit=True)),
}
TAIL = 64      # elements allocated past n: canaries past the end


def _layout_table(kind, a_e, a_h):
    from apex_dqn_amd.models.flat_params import FlatLayout, nature_segments
    rt, seg = LAYOUTS[kind]
    cfg = _cfg({**rt, "reset_interval": 5, "reset_shrink_encoder": a_e, "reset_shrink_head": a_h}, C=seg["C"], A=seg["A"])
    lay = FlatLayout(nature_segments(seg["C"], seg["A"], 64, seg.get("num_atoms", 1), noisy=seg.get("noisy", False),
                                     implicit=seg.get("implicit", False)))
    return lay, RS.reset_table(lay, cfg)


@pytest.fixture(scope="module")
def flat_state():
    """Per layout: random p, t, v, m over n + TAIL elements (the gaps and the tail are the canaries), nature32's
    padding zeroed in both nets; built once, never written."""
    out = {}
    for kind in LAYOUTS:
        lay, _ = _layout_table(kind, 0.5, 0.0)
        g = torch.Generator(device="cpu").manual_seed(3)
        arrs = [torch.randn(lay.numel + TAIL, generator=g) for _ in range(4)]
        if kind == "nature32":
            for a in arrs[:2]:
                V = lay.views(a[:lay.numel])
                V["w1"][32:] = 0
                V["b1"][32:] = 0
                V["w2"][..., 32:] = 0
        out[kind] = (lay, [a.numpy() for a in arrs])
    return out


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("kind", list(LAYOUTS))
def test_reset_kernel_against_the_mirror(flat_state, kind, split):
    """alpha pairs (0.5, 0), (0, 0), (1, 1) at r = 1 and r = 2^33: p32, t32, rms_v, rms_m bit for bit the
    mirror's, the planes byte for byte the project's split of the result inside the rows, and every element
    outside them -- each alignment gap, the TAIL elements past n -- as it was."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be = HipBackend()
    lay, host = flat_state[kind]
    n = lay.numel
    seed = RS.reset_seed(1234)
    canary = torch.full((n + TAIL,), 1.5, dtype=torch.bfloat16, device=DEV)
    for a_e, a_h, r in [(a, b, r) for a, b in ((0.5, 0.0), (0.0, 0.0), (1.0, 1.0)) for r in (1, 1 << 33)]:
        _, tab = _layout_table(kind, a_e, a_h)
        inside = torch.zeros(n + TAIL, dtype=torch.bool)
        for row in tab:
            inside[row.start:row.end] = True
        assert int((~inside[:n]).sum()) > 0                      # there are gaps to guard
        dev = [torch.from_numpy(a).to(DEV) for a in host]
        planes = [canary.clone() for _ in range(4)]
        pb, tb = (planes[0], planes[1] if split else None), (planes[2], planes[3] if split else None)
        be.reset_perturb(tab, seed, r, *(d[:n] for d in dev), tuple(None if x is None else x[:n] for x in pb),
                         tuple(None if x is None else x[:n] for x in tb))
        torch.cuda.synchronize()
        want = [a.copy() for a in host]
        RS.apply_reset(*(w[:n] for w in want), seed, r, tab)
        for name, d, w in zip(("p32", "t32", "rms_v", "rms_m"), dev, want):
            got = d.cpu().numpy()
            bad = np.flatnonzero(got.view(np.uint32) != w.view(np.uint32))
            assert bad.size == 0, (kind, name, a_e, a_h, r, bad[:8], got[bad[:8]], w[bad[:8]])
        ins = inside.to(DEV)
        for src, (hi, lo) in ((dev[0], pb), (dev[1], tb)):
            whi, wlo = _split(src, split)
            assert torch.equal(_bits(hi), _bits(torch.where(ins, whi, canary)))
            if split:
                assert torch.equal(_bits(lo), _bits(torch.where(ins, wlo, canary)))
        if not split:
            assert torch.equal(_bits(planes[1]), _bits(canary)) and torch.equal(_bits(planes[3]), _bits(canary))
        p = lay.views(dev[0][:n])
        if a_e == 1.0:
            assert np.array_equal(dev[0].cpu().numpy().view(np.uint32), host[0].view(np.uint32))
        if a_h == 0.0:
            assert torch.equal(lay.views(dev[1][:n])["wfc"], p["wfc"])        # fully reset: target = online
        if kind == "nature32":
            assert not p["w1"][32:].any() and not p["b1"][32:].any() and not p["w2"][..., 32:].any()
            assert bool(p["w1"][:32].all())


# -------------------------------------------------------------- 2. refusals
def test_launcher_refusals_launch_nothing():
    from apex_dqn_amd.ops import _lib
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be = HipBackend()
    n = 1024
    z = lambda dt=torch.float32: torch.ones(n + 4, dtype=dt, device=DEV)
    p, t, v, m = z(), z(), z(), z()
    hi, lo, th, tl = (z(torch.bfloat16) for _ in range(4))
    tab = [RS.ResetRow(0, 100, 100, 100, 0.1, 0.5, 0, 0.0), RS.ResetRow(128, 1024, 896, 896, 0.1, 0.0, 0, 0.0)]

    def args(table=tab, pb=(hi[:n], lo[:n]), tb=(th[:n], tl[:n]), pp=p[:n]):
        return be.reset_args(table, 5, 1, pp, t[:n], v[:n], m[:n], pb, tb)

    def refused(a):
        return be.lib.apex_reset_perturb(a, _lib.stream_ptr()) != 0

    a = args(pp=p[1:n + 1])                                    # a misaligned pointer (the float4 path)
    assert refused(a)
    a = args()
    a.pb = hi[1:].data_ptr()                                   # ... and a misaligned plane (packed stores)
    assert refused(a)
    assert refused(args(table=tab[::-1]))                      # an unordered table
    assert refused(args(table=[tab[0], tab[0]._replace(start=64, end=200)]))      # overlapping rows
    a = args()
    a.rows[1].end = n + 4                                      # a row past n
    assert refused(a)
    a = args()
    a.rows[1].start = 130                                      # a row off the chunk boundary
    assert refused(a)
    a = args()
    a.pb_lo = None                                             # a target lo plane without the online one
    assert refused(a)
    a = args()
    a.nrows = 0
    assert refused(a)
    a = args()
    a.rows[0].alpha = 1.5
    assert refused(a)
    torch.cuda.synchronize()
    for x in (p, t, v, m):
        assert bool((x == 1).all())
    for x in (hi, lo, th, tl):
        assert bool((x == 1).all())
    assert not refused(args())                                 # the unaltered block launches
    torch.cuda.synchronize()
    assert not v[:100].any() and bool((v[100:128] == 1).all()) and not v[128:n].any() and bool((v[n:] == 1).all())


# ------------------------------------------------------------ 3. fragments
def _frag_buffers(L):
    from apex_dqn_amd.ops import conv as C
    ws = L.ops.ws
    return [ws.get(("cf_w1frag",), C.CF_W1FRAG_BYTES, DEV, torch.uint8),
            ws.get(("cf_c2f_wfrag",), 4 * 8192 * 16, DEV, torch.uint8),
            ws.get(("cf_c3f",), C.C3F_BYTES, DEV, torch.uint8)]


@pytest.mark.parametrize("C", [1, 4])
def test_fragments_after_reset_equal_fresh_pack(C):
    """After ``reset_now`` both halves of the conv1 / C2F / C3F buffers equal a fresh pack of the new weights byte
    for byte (tests/test_gpu_target_ema.py test_target_fragments_equal_fresh_pack, for a host-side change)."""
    L = _learner({"use_graphs": False, "dtype": "fp32", "reset_interval": 1000}, C=C)
    assert L._frag_out is not None
    L.step()
    torch.cuda.synchronize()
    first = [b.clone() for b in _frag_buffers(L)]
    p_before = L.p32.clone()
    L.reset_now(1)
    torch.cuda.synchronize()
    assert not torch.equal(p_before, L.p32) and not L.rms_v.any() and not L.rms_m.any()
    bufs = _frag_buffers(L)
    got = [b.clone() for b in bufs]
    half = [1024 * C * 16, 2 * 8192 * 16, 2 * 4608 * 16]
    for name, g, f, h in zip(("conv1", "conv2", "conv3"), got, first, half):
        assert not torch.equal(g[:h], f[:h]), f"{name}: the online half never changed"
        assert not torch.equal(g[h:2 * h], f[h:2 * h]), f"{name}: the target half never changed"
    c1, c2 = L._conv12_weights()
    for sets in (2, 1):
        L.ops.conv12_pack(c1, c2, L.rt.obs_scale, sets=sets, c3=L._conv3_weights())
        torch.cuda.synchronize()
        for name, g, b in zip(("conv1", "conv2", "conv3"), got, bufs):
            assert torch.equal(g, b), f"{name} fragments differ from the pack launch (sets={sets})"


# -------------------------------------------------------------- 4. whole step
HEADS = {
    "scalar_adam_ema": {**ADAM, "target_ema_rate": 0.1},
    "c51_noisy": {"num_atoms": 51, "noisy": True},
    "iqn": {"num_atoms": 8, "dist_head": "implicit"},
}


def _step_bounds(case, u, H, T):
    """tests/test_gpu_target_ema.py's whole-step checks on one update taken by both backends from one state."""
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


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(HEADS))
def test_seven_updates_hip_vs_torch_backend(case, dtype):
    """I = 3, seven updates at B = 16: every update of the HIP step against the torch backend with the bounds of
    tests/test_gpu_target_ema.py test_two_updates_hip_vs_torch_backend, each taken by both backends from one state
    (the torch learner starts an update from the HIP learner's state, as there, for the reason given there).
    At updates 3 and 6 each backend resets its own state: the kernel's result is the mirror applied to the HIP
    learner's state before it, bit for bit, and so is the torch backend's."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    I = 3
    split = dtype == "fp32"
    Ls = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        cfg = _cfg({**HEADS[case], "dtype": dtype, "use_graphs": False, "reset_interval": I, "seed": 5}, B=16,
                   q_target_sync_freq=3)
        L = FusedNatureLearner(cfg, DEV, _replay(), backend=be, split=split)
        if be == "torch":
            L.ops.dtype = torch.float32
        Ls[be] = L
    H, T = Ls["hip"], Ls["torch"]
    tab, seed = H._reset_table, H._seed_r
    for u in range(7):
        if u > 0:
            for name in ("p32", "_pbf_all", "rms_v", "rms_m", "t32", "_tbf_all"):
                getattr(T, name).copy_(getattr(H, name))
            for name in ("leaf", "nodes", "min_bits"):
                getattr(T.replay, name).copy_(getattr(H.replay, name))
            T._online_changed()
            T._target_changed()
        H._sample()
        T._sample()
        assert torch.equal(H.S["idx"], T.S["idx"]), u
        boundary = (u + 1) % I == 0
        if boundary:       # hold the reset back for this step(), to read the state the update leaves: the boundary
            for L in Ls.values():      # work (sync, then reset) runs below, where step() would have run it
                L.reset_I = 0
        H.step()
        T.step()
        torch.cuda.synchronize()
        _step_bounds(f"{case}/{dtype}", u, H, T)
        if boundary:
            for be, L in Ls.items():
                L.reset_I = I
                want = [x.cpu().numpy().copy() for x in (L.p32, L.t32, L.rms_v, L.rms_m)]
                RS.apply_reset(*want, seed, (u + 1) // I, tab)
                L._boundary_work()
                torch.cuda.synchronize()
                for name, w in zip(("p32", "t32", "rms_v", "rms_m"), want):
                    assert np.array_equal(getattr(L, name).cpu().numpy().view(np.uint32), w.view(np.uint32)), (be, u, name)
                hi, lo = _split(L.p32, split)
                assert torch.equal(L.pbf.float(), hi.float()) and (not split or torch.equal(L.pbf_lo.float(), lo.float()))
                hi, lo = _split(L.t32, split)
                assert torch.equal(L.tbf.float(), hi.float()) and (not split or torch.equal(L.tbf_lo.float(), lo.float()))
                assert int(L.upd_t0) == u + 1 and torch.equal(L.T["wfc"], L.P["wfc"])
    assert H.last_metrics()["resets"] == 2 == T.last_metrics()["resets"]


# ------------------------------------------------------------------ 5. graphs
class _Counting:
    def __init__(self, graph):
        self.graph, self.n = graph, 0

    def replay(self):
        self.n += 1
        return self.graph.replay()


def _state(L):
    return [t.clone() for t in (L.p32, L.t32, L._pbf_all, L._tbf_all, L.rms_v, L.rms_m)] + \
        [b.clone() for b in _frag_buffers(L)]


GRAPH_RT = {**ADAM, "dtype": "fp32", "graph_steps": 2, "reset_interval": 4, "target_ema_rate": 0.1}


def test_graphs_break_at_reset_boundaries_and_equal_eager():
    """graph_steps = 2, I = 4, steps(8) with the soft target (no sync boundary): four replays of the 2-update graph,
    no single step, no recapture; the result is eight eager step() calls bit for bit -- parameters, target, planes,
    moments, fragments, and the replay's leaves and draw counter (tests/test_gpu_target_ema.py's comparison)."""
    G = _learner({**GRAPH_RT, "use_graphs": True}, q_target_sync_freq=1000)
    G.prepare_graphs(multi=True)
    captures = G.graph_captures
    multi, single = _Counting(G._multi), _Counting(G._graphs)
    G._multi, G._graphs = multi, single
    G.steps(8)
    torch.cuda.synchronize()
    assert (multi.n, single.n) == (4, 0) and G.num_q_updates == G.update_index() == 8
    assert G.graph_captures == captures and int(G.upd_t0) == 8 and G.last_metrics()["resets"] == 2
    G._multi, G._graphs = multi.graph, single.graph
    E = _learner({**GRAPH_RT, "use_graphs": False}, q_target_sync_freq=1000)
    for _ in range(8):
        E.step()
    torch.cuda.synchronize()
    names = ("p32", "t32", "_pbf_all", "_tbf_all", "rms_v", "rms_m", "conv1 frags", "conv2 frags", "conv3 frags")
    for name, a, b in zip(names, _state(G), _state(E)):
        assert torch.equal(a, b), name
    assert torch.equal(G.replay.leaf, E.replay.leaf) and torch.equal(G.replay.ctr, E.replay.ctr)
    assert not G.rms_v.any() and torch.equal(G.T["wfc"], G.P["wfc"]) and not torch.equal(G.T["w3"], G.P["w3"])


def test_replayed_graph_reads_the_reset_word():
    """The first update after a reset, replayed from the captured one-update graph: the parameters moved by
    lr (m / c1) / (sqrt(v / c2) + eps) with the mirror's corrections at t = 1, evaluated in numpy fp32 from the
    device's own moments -- and not with those of t = 5, which a graph that ignored ``t0`` would use."""
    G = _learner({**GRAPH_RT, "use_graphs": True}, q_target_sync_freq=1000)
    G.steps(4)
    torch.cuda.synchronize()
    assert int(G.upd_t0) == 4 and not G.rms_m.any()
    p4 = G.p32.cpu().numpy().copy()
    single = _Counting(G._graphs)
    G._graphs = single
    G.steps(1)
    torch.cuda.synchronize()
    G._graphs = single.graph
    assert single.n == 1 and G.update_index() == 5
    m, v, p5 = (x.cpu().numpy() for x in (G.rms_m, G.rms_v, G.p32))
    rt = G.rt
    lr = sch.lr_at(4, rt.lr, rt.lr_warmup_steps, rt.lr_decay_steps, rt.lr_end)
    moved = {}
    for t0 in (4, 0):
        c1, c2 = sch.adam_corrections(4, rt.adam_beta1, rt.adam_beta2, t0=t0)
        moved[t0] = p4 - lr * (m / c1) / (np.sqrt(v / c2) + f32(rt.adam_eps))
    assert sch.adam_corrections(4, rt.adam_beta1, rt.adam_beta2, t0=4)[0] == f32(1 - rt.adam_beta1)
    assert m.any() and not np.array_equal(p5, p4)
    # one rounding of the final subtraction apart at most (the kernel's own fp32 operations, in its order); an
    # element without gradient (m = v = 0) stays where it was under either count
    tol = 2.0 ** -23 * np.abs(p5).max()
    np.testing.assert_allclose(p5, moved[4], rtol=0, atol=tol)
    assert np.abs(p5 - moved[0]).max() > 100 * tol


# ------------------------------------------------------------------ 6. resume
def test_gpu_resume_across_a_boundary(tmp_path):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg = _cfg({**ADAM, "use_graphs": True, "graph_steps": 2, "reset_interval": 3, "noisy": True}, q_target_sync_freq=3)
    rp = _replay(seed=5)
    torch.manual_seed(0)
    L = FusedNatureLearner(cfg, DEV, rp)
    for _ in range(4):
        L.step()
    torch.cuda.synchronize()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    L.steps(3)
    torch.cuda.synchronize()
    rp2 = _replay(seed=5)
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.num_q_updates == L2.update_index() == 4 and int(L2.upd_t0) == 3
    L2.steps(3)
    torch.cuda.synchronize()
    assert int(L2.upd_t0) == 6 == int(L.upd_t0)
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (L._pbf_all, L2._pbf_all),
                 (L._tbf_all, L2._tbf_all), (rp.leaf, rp2.leaf), (rp.ctr, rp2.ctr), (L.td_abs, L2.td_abs)):
        assert torch.equal(a, b)


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
                                            "env_backend": "fake_ale", "reset_interval": 20}})
    out = train_frames(cfg, DEV, 50, num_envs=16, async_actors=False)
    L = out["learner"]
    torch.cuda.synchronize()
    assert L.reset_I == 20 and L.num_q_updates == L.update_index() == 50 and int(L.upd_t0) == 40
    m = L.last_metrics()
    assert m["resets"] == 2 and np.isfinite(m["loss"]) and m["grad_norm"] > 0
    assert bool(torch.isfinite(L.td_abs).all()) and np.isfinite(out["losses"]).all()
    hi, lo = _split(L.p32, L.split)
    assert torch.equal(L.pbf.float(), hi.float()) and torch.equal(L.pbf_lo.float(), lo.float())
    # the next publish hands the actors the planes the learner holds
    G = out["actors"]
    G.sync_params()
    torch.cuda.synchronize()
    assert torch.equal(G.p32, L.p32)
    assert torch.equal(_bits(G._pbf_all), _bits(L._pbf_all if G.split else L.pbf))
