"""Adam and the step-indexed lr / IS-exponent schedules on the CPU: config checks, the
host mirror (learner/schedules.py), the torch backend's Adam against ``torch.optim.Adam``,
the learners' device-resident update index, checkpoints, and a gloo data-parallel run."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import schedules as sch

ENV = {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. config
@pytest.mark.parametrize("rt", [{"optimizer": "sgd"}, {"lr_end": 1e-5}, {"lr_decay_steps": 10},
                                {"is_beta_end": 1.0}, {"is_beta_anneal_steps": 10},
                                {"is_beta_end": 1.0, "is_beta_anneal_steps": 10, "use_is_weights": False}])
def test_config_refuses_inconsistent_keys(rt):
    with pytest.raises(ValueError):
        ApexConfig.from_dict({"Runtime": rt})


def test_config_defaults_and_reference_parameters():
    cfg = ApexConfig.load(os.path.join(ROOT, "configs", "reference_parameters.json"))
    rt = cfg.Runtime
    assert rt.optimizer == "rmsprop" and rt.lr_end is None and rt.is_beta_end is None
    assert rt.lr_warmup_steps == rt.lr_decay_steps == rt.is_beta_anneal_steps == 0
    assert (rt.adam_beta1, rt.adam_beta2, rt.adam_eps) == (0.9, 0.999, 1.5e-4)
    ok = ApexConfig.from_dict({"Runtime": {"optimizer": "adam", "lr_warmup_steps": 3, "lr_decay_steps": 5,
                                           "lr_end": 1e-5, "is_beta_end": 1.0, "is_beta_anneal_steps": 7}})
    assert ok.Runtime.optimizer == "adam"


# ------------------------------------------------------------------ 2. mirror
def test_mirror_values_at_the_edges():
    lr, end, W, D = 2.5e-4, 1e-5, 4, 10
    f32 = np.float32
    assert sch.lr_at(0, lr, W, D, end) == f32(lr / 4)
    assert sch.lr_at(W - 1, lr, W, D, end) == f32(lr)                 # (u + 1) / warmup = 1
    assert sch.lr_at(W, lr, W, D, end) == f32(lr)                     # ramp starts at lr
    assert sch.lr_at(W + 5, lr, W, D, end) == f32(lr + (end - lr) * 0.5)
    assert sch.lr_at(W + D, lr, W, D, end) == f32(end)
    assert sch.lr_at(W + D + 1000, lr, W, D, end) == f32(end)
    assert sch.lr_at(7, lr) == f32(lr) and sch.lr_at(0, lr, W) == f32(lr / 4) and sch.lr_at(W, lr, W) == f32(lr)
    b0, b1, S = 0.4, 1.0, 5
    assert sch.beta_at(0, b0, b1, S) == f32(b0)
    assert sch.beta_at(S - 1, b0, b1, S) == f32(b0 + (b1 - b0) * 0.8)
    assert sch.beta_at(S, b0, b1, S) == f32(1.0) and sch.beta_at(S + 99, b0, b1, S) == f32(1.0)
    assert sch.beta_at(3, b0) == f32(b0)
    # the tensor form the torch paths use is the same arithmetic
    ctr, base = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    spec = sch.OptSpec("adam", ctr, base, lr, W, D, end)
    for u in (0, W - 1, W, W + 3, W + D, W + D + 50):
        ctr.fill_(u + 1)
        assert float(spec.lr_tensor()) == float(sch.lr_at(u, lr, W, D, end))
    c1, c2 = sch.adam_corrections(0, 0.9, 0.999)
    assert c1 == f32(1 - 0.9) and c2 == f32(1 - 0.999)
    # (the squaring chain's roundings are amplified by up to t: t * 2^-53 relative)
    assert abs(float(sch.pow_int(0.999, 1000)) / 0.999 ** 1000 - 1) < 1000 * 2.0 ** -53


# ------------------------------------------------------------ 3. Adam numerics
ADAM = dict(lr=2.5e-4, b1=0.9, b2=0.999, eps=1.5e-4, clip=40.0, warmup=2, decay=3, lr_end=2.5e-5)


def adam_problem(n, updates=6, seed=1):
    """Parameters and ``updates`` gradients (the second one large: the clip engages), with
    the fp64 ``torch.optim.Adam`` + ``clip_grad_norm_`` trajectory under the lr schedule."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.5 if it == 1 else 0.01) for it in range(updates)]
    tp = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([tp], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    norms = []
    for u, gr in enumerate(grads):
        tp.grad = gr.double().clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([tp], ADAM["clip"])))
        for grp in opt.param_groups:
            grp["lr"] = float(sch.lr_at(u, ADAM["lr"], ADAM["warmup"], ADAM["decay"], ADAM["lr_end"]))
        opt.step()
    assert norms[1] > ADAM["clip"] > norms[0]
    return p0, grads, tp.detach().clone()


def adam_spec(device="cpu"):
    ctr = torch.zeros(1, dtype=torch.int64, device=device)
    base = torch.zeros(1, dtype=torch.int64, device=device)
    return sch.OptSpec("adam", ctr, base, ADAM["lr"], ADAM["warmup"], ADAM["decay"], ADAM["lr_end"], ADAM["b1"],
                       ADAM["b2"], ADAM["eps"])


def numpy_adam_step(p, g, m, v, u, clip=ADAM["clip"], gscale=np.float32(1.0)):
    """One update of the kernel's formula (csrc/rmsprop_common.h OPT_ADAM) in numpy fp32."""
    f32 = np.float32
    norm = f32(np.sqrt(np.sum(g.astype(np.float64) ** 2))) * gscale
    coef = gscale * (min(f32(1.0), f32(clip) / (norm + f32(1e-6))) if clip > 0 else f32(1.0))
    lr = sch.lr_at(u, ADAM["lr"], ADAM["warmup"], ADAM["decay"], ADAM["lr_end"])
    c1, c2 = sch.adam_corrections(u, ADAM["b1"], ADAM["b2"])
    b1, b2 = f32(ADAM["b1"]), f32(ADAM["b2"])
    gg = g * coef
    m[:] = b1 * m + (f32(1) - b1) * gg
    v[:] = b2 * v + (f32(1) - b2) * gg * gg
    p -= lr * (m / c1) / (np.sqrt(v / c2) + f32(ADAM["eps"]))


def test_torch_backend_adam_vs_torch_optim_adam():
    """Six updates, clip engaged on one, warmup 2 + decay 3: the torch backend's Adam against
    fp64 ``torch.optim.Adam`` at the RMSprop kernel test's tolerances -- and the kernel's
    formula evaluated in numpy fp32 within 3 % of them, which is the headroom the fp32
    arithmetic leaves."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    n = 200_003
    p0, grads, ref = adam_problem(n)
    spec = adam_spec()
    be = TorchBackend()
    p, v, m = p0.clone(), torch.zeros(n), torch.zeros(n)
    pbf, norm = torch.zeros(n), torch.zeros(1)
    pn, mn, vn = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for u, gr in enumerate(grads):
        spec.ctr += 1                      # the priority write-back's bump precedes the optimizer
        be.optimizer(p, gr, v, m, pbf, ADAM["lr"], 0.95, 1.5e-7, ADAM["clip"], True, None, norm, opt=spec)
        numpy_adam_step(pn, gr.numpy(), mn, vn, u)
        torch.testing.assert_close(norm[0], gr.double().norm().float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(p, ref.float(), rtol=1e-5, atol=1e-6)
    assert torch.equal(pbf, p)
    err = np.abs(pn.astype(np.float64) - ref.numpy())
    assert (err <= 0.03 * (1e-6 + 1e-5 * np.abs(ref.numpy()))).all(), float(err.max())
    # the backend and the numpy evaluation are the same fp32 arithmetic
    np.testing.assert_allclose(p.numpy(), pn, rtol=1e-6, atol=1e-8)


# ------------------------------------------------- 4. learner: index and beta(u)
def _replay(K=200, cap=400, seed=0, A=6):
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    rp = GpuReplayShard(cap, cap, cap + 200, 4, device="cpu", seed=seed + 3)
    rng = np.random.default_rng(seed)
    seqs = rp.append_frames(rng.integers(0, 255, (K + 100, 84, 84), dtype=np.uint8))
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    nx = np.stack([seqs[i + 3:i + 7] for i in range(K)])
    g = np.full(K, 0.97)
    g[::5] = 0.0
    rp.insert(dict(S_t=st, S_tpn=nx, A_t=rng.integers(0, A, K), R=rng.normal(size=K) * 3, Gamma=g,
                   priority=rng.random(K)))
    return rp


RT_ADAM = {"optimizer": "adam", "lr_warmup_steps": 2, "lr_decay_steps": 3, "lr_end": 2.5e-5, "grad_clip": 40.0,
           "is_beta_end": 1.0, "is_beta_anneal_steps": 5}


def _cfg(rt, B=8, **learner):
    return ApexConfig.from_dict({"env_conf": ENV, "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"use_graphs": False, **rt}})


def _record_batches(L, rec):
    """Record the batch every update consumes (at its head launch) with the weights the host
    formula gives for it from the leaves it was drawn from."""
    orig, rp, rt = L.ops.head, L.replay, L.rt

    def head(*a, **k):
        S, u = L.S, L.num_q_updates
        beta = torch.tensor(sch.beta_at(u, rp.beta, rt.is_beta_end, rt.is_beta_anneal_steps))
        p = rp.leaf[S["idx"]].float()
        want = (p / max(rp.min_leaf(), 1e-38)).pow(-beta).clamp(max=1.0)
        rec.append((S["idx"].clone(), S["weights"].clone(), want))
        return orig(*a, **k)

    L.ops.head = head


def test_learner_beta_schedule_and_update_index():
    """Adam + beta annealed over 5 updates on the CPU learner: the batch update u consumes
    carries (p / p_min)^-beta(u) whether it was pre-sampled inside update u - 1 or drawn at
    the head of u, both draw the same batches, and the device counter tracks num_q_updates."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    runs = {}
    for pre in (True, False):
        torch.manual_seed(0)
        L = FusedNatureLearner(_cfg({**RT_ADAM, "presample": pre}), "cpu", _replay())
        assert L._opt is not None and L._opt.adam and L.replay.beta_sched is not None
        rec = []
        _record_batches(L, rec)
        assert L.update_index() == 0
        for u in range(8):
            L.step()
            assert L.update_index() == L.num_q_updates == u + 1
            idx, w, want = rec[u]
            assert torch.equal(w, want), (pre, u)
        betas = [float(sch.beta_at(u, 0.4, 1.0, 5)) for u in range(8)]
        assert betas[0] == float(np.float32(0.4)) and betas[5] == betas[7] == 1.0 and betas[1] > betas[0]
        runs[pre] = (rec, L.p32.clone(), L.rms_m.clone(), L.rms_v.clone())
        m = L.schedule_metrics()
        assert m["lr"] == float(sch.lr_at(7, L.rt.lr, 2, 3, 2.5e-5)) and m["is_beta"] == 1.0
    for (ia, wa, _), (ib, wb, _) in zip(runs[True][0], runs[False][0]):
        assert torch.equal(ia, ib) and torch.equal(wa, wb)
    for a, b in zip(runs[True][1:], runs[False][1:]):
        assert torch.equal(a, b)


def test_default_config_issues_no_schedule():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    L = FusedNatureLearner(_cfg({}), "cpu", _replay())
    assert L._opt is None and L._opt_kw() == {} and L.replay.beta_sched is None
    L.step()
    assert L.update_index() == 1


# ---------------------------------------------------------- 5. checkpoints
def test_adam_resume_matches_uninterrupted_run(tmp_path):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg = _cfg(RT_ADAM, q_target_sync_freq=2)
    torch.manual_seed(0)
    rp = _replay()
    L = FusedNatureLearner(cfg, "cpu", rp)
    for _ in range(3):
        L.step()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(3):
        L.step()
    rp2 = _replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), "cpu", rp2)
    assert L2.num_q_updates == L2.update_index() == 3
    for _ in range(3):
        L2.step()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.S["weights"], L2.S["weights"])):
        assert torch.equal(a, b)


def test_rmsprop_checkpoint_into_adam_learner_starts_state_fresh(tmp_path, capsys):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(0)
    R = FusedNatureLearner(_cfg({}), "cpu", _replay())
    R.step()
    ck = str(tmp_path / "rms.pt")
    R.save(ck)
    assert torch.load(ck, weights_only=True)["optimizer_state"]["kind"] == "rmsprop"
    A = FusedNatureLearner(_cfg(RT_ADAM), "cpu", _replay())
    A.step()                                   # (non-zero Adam state that the load must clear)
    capsys.readouterr()
    assert A.load(ck)
    out = capsys.readouterr().out
    assert "rmsprop" in out and "adam" in out and "WARNING" in out
    assert torch.equal(A.p32, R.p32) and A.num_q_updates == A.update_index() == 1
    assert not A.rms_m.any() and not A.rms_v.any()
    # an untagged (older) state counts as rmsprop: an RMSprop learner restores it
    from apex_dqn_amd.utils.checkpoint import optimizer_state_kind
    assert optimizer_state_kind({"rms_v": R.rms_v}) == "rmsprop"
    R2 = FusedNatureLearner(_cfg({}), "cpu", _replay())
    assert R2.load(ck) and torch.equal(R2.rms_v, R.rms_v)


# ------------------------------------------- 6. the other learners (two updates)
def _check_two_adam_updates(L):
    for u in range(2):
        p, m, v = (t.numpy().copy() for t in (L.p32, L.rms_m, L.rms_v))
        L.step()
        numpy_adam_step(p, L.g32.numpy().copy(), m, v, u)
        np.testing.assert_allclose(L.p32.numpy(), p, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(L.rms_m.numpy(), m, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(L.rms_v.numpy(), v, rtol=1e-6, atol=1e-12)
        assert L.update_index() == L.num_q_updates == u + 1


RT_OTHER = {"optimizer": "adam", "lr": ADAM["lr"], "lr_warmup_steps": 2, "lr_decay_steps": 3, "lr_end": 2.5e-5, "grad_clip": 40.0,
            "is_normalise": "global_min"}


def test_impala_learner_adam_two_updates():
    from apex_dqn_amd.learner.impala_learner import FusedImpalaLearner
    torch.manual_seed(0)
    L = FusedImpalaLearner(_cfg({**RT_OTHER, "network": "impala"}, B=4), "cpu", _replay(K=150, cap=256))
    _check_two_adam_updates(L)


def test_graph_learner_adam_two_updates():
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    torch.manual_seed(0)
    L = GraphLearner(_cfg(RT_OTHER, B=4), "cpu", _replay(K=150, cap=256))
    _check_two_adam_updates(L)


# ------------------------------------------------------- 7. gloo, two ranks
CAP, FR, BG, STEPS = 300, 400, 16, 3
RT_DP = {"optimizer": "adam", "lr_warmup_steps": 2, "lr_decay_steps": 2, "lr_end": 2.5e-5, "is_beta_end": 1.0,
         "is_beta_anneal_steps": 2}


def _dp_shard(rank):
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    rp = GpuReplayShard(CAP, CAP, FR, 4, device="cpu", seed=rank + 3)
    rng = np.random.default_rng(100 + rank)
    seqs = rp.append_frames(rng.integers(0, 255, (120, 84, 84), dtype=np.uint8))
    K = 100
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, 5, K), R=rng.normal(size=K),
                   Gamma=np.where(rng.random(K) < 0.2, 0.0, 0.97), priority=rng.random(K) * (1 + 0.5 * rank)))
    return rp


def _dp_concat(world):
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    shards = [_dp_shard(r) for r in range(world)]
    rp = GpuReplayShard(CAP * world, CAP * world, FR * world, 4, device="cpu", seed=3)
    rp.frames.copy_(torch.cat([s.frames for s in shards]))
    for name in ("act", "rew", "gam", "gen", "leaf"):
        getattr(rp, name).copy_(torch.cat([getattr(s, name) for s in shards]))
    rp.obs.copy_(torch.cat([s.obs + r * FR for r, s in enumerate(shards)]))
    rp.nxt.copy_(torch.cat([s.nxt + r * FR for r, s in enumerate(shards)]))
    rp.live = rp.head = CAP * world
    rp._torch_rebuild()
    return rp


def _dp_worker(rank, world, concat, path, q):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.parallel.dist import Comm
    torch.set_num_threads(2)
    comm = Comm.init(rank, world, f"file://{path}", backend="gloo", force=True)
    torch.manual_seed(1234)
    rp = _dp_concat(concat) if concat else _dp_shard(rank)
    cfg = ApexConfig.from_dict({"env_conf": {**ENV, "action_dim": 5},
                                "Learner": {"replay_sample_size": BG, "q_target_sync_freq": 2},
                                "Runtime": {"use_graphs": False, "grad_clip": 40.0, "force_dp": True, "seed": 7 * rank,
                                            "batch_scope": "global", "dp_batch_slack": 1.0,
                                            "dp_fc_exchange": "factors" if world > 1 else "allreduce",
                                            "dp_shard_update": "auto", **RT_DP}})
    L = FusedNatureLearner(cfg, "cpu", rp, comm=comm)
    assert L._shard == (world > 1)
    mask = np.ones(L.g32.numel(), bool)
    if L._shard:                      # the entries this rank computes (its own fc rows)
        off = L.layout.offsets
        mask[off["wfc"]:] = False
        o = off["wfc"] + L._fc_r0 * 3136
        mask[o:o + L._fc_S * 3136] = True
        mask[off["bfc"] + L._fc_r0:off["bfc"] + L._fc_r0 + L._fc_S] = True
    grads, wsum = [], []
    for u in range(STEPS):
        L.refresh_replay_stats()
        L._sample()
        w = L.S["weights"]
        # (without the W B / M factor of the sharded draw: the bare (p / p_min)^-beta(u))
        wsum.append((float(w.sum() / L.S["wscale"][0]), int((w > 0).sum())))
        L.step()
        grads.append(np.where(mask, L.g32.numpy(), np.nan))
        assert L.update_index() == L.num_q_updates
    L.materialize()
    q.put((rank, grads, L.p32.numpy().copy(), wsum))
    comm.shutdown()


def _dp_run(world, concat):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        procs = [ctx.Process(target=_dp_worker, args=(r, world, concat, os.path.join(td, "store"), q))
                 for r in range(world)]
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in range(world)]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    return sorted(res, key=lambda r: r[0])


@pytest.mark.slow
def test_gloo_two_ranks_adam_with_schedules():
    """W = 2 (factors, sharded update) with Adam and both schedules: replicas bit-identical,
    and against the one-rank run over the concatenated replay the parameters differ by no
    more than Adam can move them for the recorded gradient differences: one update moves a
    parameter by lr (m / c1) / (sqrt(v / c2) + eps), at most lr / eps per unit of gradient
    difference in m / c1 (the denominator's own change only shrinks a step), doubled for
    the second-moment term; summed over the updates."""
    multi = _dp_run(2, 0)
    one = _dp_run(1, 2)[0]
    assert np.array_equal(multi[0][2], multi[1][2])
    # the sharded draw carries the annealed exponent: same global batch, same weights' sum
    for s in range(STEPS):
        n = sum(r[3][s][1] for r in multi)
        assert n == one[3][s][1] == BG
        assert abs(sum(r[3][s][0] for r in multi) - one[3][s][0]) <= 1e-5 * BG
    gdiff = 0.0
    for r in multi:
        for s in range(STEPS):
            m = ~np.isnan(r[1][s])
            gdiff = max(gdiff, float(np.abs(r[1][s][m] - one[1][s][m]).max()))
    lr_sum = sum(float(sch.lr_at(s, 0.00025 / 4, 2, 2, 2.5e-5)) for s in range(STEPS))
    bound = 2.0 * lr_sum / 1.5e-4 * gdiff + 1e-6
    for r in multi:
        dp = float(np.abs(r[2] - one[2]).max())
        assert dp <= bound, (dp, bound, gdiff)
