"""Adam and the step-indexed lr / IS-exponent schedules on the GPU: the optimizer kernels'
Adam variant (csrc/rmsprop_common.h OPT_ADAM) in every launch form, and the learner's
device-resident update index inside replayed graphs, the DP step and a resume."""
import ctypes

import numpy as np
import pytest
import torch

from test_opt_schedules_cpu import ADAM, adam_problem, adam_spec

from apex_dqn_amd.learner import schedules as sch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ENV = {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"}
RT = {"optimizer": "adam", "lr_warmup_steps": 3, "lr_decay_steps": 6, "lr_end": 1e-5, "is_beta_end": 1.0,
      "is_beta_anneal_steps": 7, "graph_steps": 4}


def _fill(rp, K=1500, seed=11, A=6):
    rng = np.random.default_rng(seed)
    seqs = rp.append_frames(rng.integers(0, 255, (K + 8, 84, 84), dtype=np.uint8))
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, A, K), R=rng.normal(size=K).astype(np.float32),
                   Gamma=np.where(rng.random(K) < 0.1, 0.0, 0.97).astype(np.float32),
                   priority=rng.random(K).astype(np.float32) * 3 + 0.01))
    return seqs


def _replay(seed=7):
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=seed)
    _fill(rp)
    return rp


def _cfg(rt, B=64, **learner):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": ENV, "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {**RT, **rt}})


# ------------------------------------------------------------------ 1. kernel
@pytest.fixture(scope="module")
def problem():
    """n = 1,048,583: not a multiple of 4 and more than 2 x 4 x 256 x 512 elements, so the
    peeled first chunk, the steady loop and the scalar tail of the body all run."""
    return adam_problem(1_048_583)


@pytest.mark.parametrize("split", [False, True])
def test_adam_kernel_vs_torch_optim_adam(problem, split):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    p0, grads, ref = problem
    n = p0.numel()
    be, spec = HipBackend(), adam_spec(DEV)
    p, v, m = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hi = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    lo = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if split else None
    parts, norm = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    for gr in grads:
        spec.ctr += 1
        g = gr.to(DEV)
        be.optimizer(p, g, v, m, hi, ADAM["lr"], 0.95, 1.5e-7, ADAM["clip"], True, parts, norm, pb_lo=lo, opt=spec)
        torch.testing.assert_close(norm[0], g.double().norm().float(), rtol=1e-5, atol=1e-6)
    torch.cuda.synchronize()
    torch.testing.assert_close(p.cpu(), ref.float(), rtol=1e-5, atol=1e-6)
    assert torch.equal(hi, p.to(torch.bfloat16))
    if split:
        # hi + lo: bf16 rounds to 2^-9 relative, twice -> 2^-18 of |p| (2^-17: margin for the
        # rounding of the residual's own exponent)
        err = (hi.double() + lo.double() - p.double()).abs()
        assert bool((err <= 2.0 ** -17 * p.double().abs() + 1e-30).all()), float(err.max())


# ------------------------------------------------------------ 2. launch forms
def _forms_state(n, device=DEV):
    g = torch.Generator(device="cpu").manual_seed(1)
    return torch.randn(n, generator=g).to(device), (torch.randn(n, generator=g) * 1e-2).to(device)


def test_adam_launch_forms_bit_identical():
    """Plain launch, producer-partials launch and the fused optimizer + sample launch take
    the same Adam update (and the fused one draws the batch a separate sample launch
    draws, with the annealed exponent); a ``segs`` launch equals them on its ranges."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    n, B = 100_003, 64
    p0, gr = _forms_state(n)
    be = HipBackend()
    res = {}
    off2 = 60_000
    segs = [(0, 30_000), (off2, n - off2)]
    for form in ("plain", "partials", "fused", "segs"):
        rp = _replay(seed=4)
        spec = adam_spec(DEV)
        spec.ctr, spec.base = rp.ctr, torch.zeros(1, dtype=torch.int64, device=DEV)
        rp.set_beta_schedule(spec.base, 1.0, 4)
        p, v, m = p0.clone(), torch.full((n,), 1e-6, device=DEV), torch.full((n,), 1e-4, device=DEV)
        pbf = torch.zeros(n, device=DEV, dtype=torch.bfloat16)
        part, gn = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
        S = rp.alloc_sample_buffers(B)
        nxt2 = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
        args = (p, gr, v, m, pbf, ADAM["lr"], 0.95, 1.5e-7, ADAM["clip"], True, part, gn)
        for _ in range(2):                    # two updates: u = 0 and 1 of the schedules
            rp.ctr += 1
            if form == "plain":
                be.optimizer(*args, opt=spec)
            else:
                np_ = be.grad_sqnorm_partials(gr, part)
                kw = dict(norm_total=(part, np_), opt=spec)
                if form == "partials":
                    be.optimizer(*args, **kw)
                else:
                    be.optimizer(*args, sample=(rp, B, S, nxt2), **kw, **({"segs": segs} if form == "segs" else {}))
            if form in ("plain", "partials"):
                rp.sample(B, out=S, nxt2=nxt2)
        torch.cuda.synchronize()
        res[form] = (p, v, m, pbf, gn, S, nxt2)
    a = res["plain"]
    for form in ("partials", "fused"):
        b = res[form]
        for x, y in zip(a[:5], b[:5]):
            assert torch.equal(x, y), form
        for k in a[5]:
            assert torch.equal(a[5][k], b[5][k]), (form, k)
        assert torch.equal(a[6], b[6])
    s = res["segs"]
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for o, ln in segs:
        mask[o:o + ln] = True
    init = (p0, torch.full((n,), 1e-6, device=DEV), torch.full((n,), 1e-4, device=DEV))
    for k in range(3):
        assert torch.equal(s[k][mask], a[k][mask]) and torch.equal(s[k][~mask], init[k][~mask]), k
    assert torch.equal(s[3][mask], a[3][mask]) and torch.equal(s[4], a[4])
    # the drawn weights are the annealed (p / p_min)^-beta(2) (powf on the device: 1e-5)
    idx = a[5]["idx"].cpu()
    leaf = rp.leaf.cpu().double()
    want = (leaf[idx] / rp.min_leaf()).pow(-float(sch.beta_at(2, rp.beta, 1.0, 4))).clamp(max=1.0)
    torch.testing.assert_close(a[5]["weights"].cpu().double(), want, rtol=1e-5, atol=0)


def _learner(rt, rp=None, B=64, **learner):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(0)
    return FusedNatureLearner(_cfg(rt, B, **learner), DEV, rp if rp is not None else _replay(), backend="hip")


def test_adam_frag_out_equals_fresh_pack():
    """The Adam launch ends in the same fragment stores: after real updates the fused
    forward's conv1 / conv2 / conv3 operands equal a fresh pack of the updated weights."""
    from apex_dqn_amd.ops import conv as C
    L = _learner({"use_graphs": False, "dtype": "fp32"})
    assert L._frag_out is not None and L._opt is not None and L._opt.adam
    for _ in range(2):
        L.step()
    torch.cuda.synchronize()
    ws = L.ops.ws
    bufs = [ws.get(("cf_w1frag",), C.CF_W1FRAG_BYTES, DEV, torch.uint8),
            ws.get(("cf_c2f_wfrag",), 4 * 8192 * 16, DEV, torch.uint8),
            ws.get(("cf_c3f",), C.C3F_BYTES, DEV, torch.uint8)]
    got = [b.clone() for b in bufs]
    c1, c2 = L._conv12_weights()
    L.ops.conv12_pack(c1, c2, L.rt.obs_scale, sets=1, c3=L._conv3_weights())
    torch.cuda.synchronize()
    for name, g, b in zip(("conv1", "conv2", "conv3"), got, bufs):
        assert torch.equal(g, b), f"{name} fragments differ from the pack launch"


# ------------------------------------------- 3. graphs == eager, beta(u) weights
def _want_weights(rp, S, u, rt):
    """Host formula for the batch in ``S`` drawn from the replay's current leaves for update u."""
    idx = S["idx"].cpu()
    leaf = rp.leaf.cpu().double()
    beta = float(sch.beta_at(u, rp.beta, rt.is_beta_end, rt.is_beta_anneal_steps))
    return (leaf[idx] / rp.min_leaf()).pow(-beta).clamp(max=1.0)


def _mutate(rp):
    """New transitions + an exact rebuild between two chunks: the version bump forces a fresh
    draw at the head of the next update."""
    rng = np.random.default_rng(5)
    seqs = rp.append_frames(rng.integers(0, 255, (60, 84, 84), dtype=np.uint8))
    K = 50
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, 6, K), R=rng.normal(size=K).astype(np.float32),
                   Gamma=np.full(K, 0.97, np.float32), priority=rng.random(K).astype(np.float32) + 0.5))
    rp.rebuild()


class _Weights:
    """Every update's pre-sampled weights, copied from inside the multi-update graph."""

    def __init__(self, L, k):
        self.L, self.w = L, [torch.zeros_like(L.S["weights"]) for _ in range(k)]

    def __call__(self, i):
        self.w[i].copy_(self.L.S["weights"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_steps_equal_eager_steps_with_schedules(dtype):
    """steps(5) + new transitions + steps(6) with graphs (multi-update graphs of 4 and
    one-update graphs) against the same eleven eager step() calls: parameters, Adam
    moments, the counter and every update's weights bit-identical; the weights are the
    host's (p / p_min)^-beta(u)."""
    out = {}
    for graphs in (True, False):
        L = _learner({"use_graphs": graphs, "dtype": dtype}, q_target_sync_freq=1000)
        rp, rt = L.replay, L.rt
        ws = []
        if graphs:
            tr = _Weights(L, 4)
            L._step_hook = tr
            L.prepare_graphs(multi=True)
            assert L._multi is not None and L.update_index() == 0

        def run(n):
            if not graphs:
                for _ in range(n):
                    L.step()
                    torch.cuda.synchronize()
                    # (eager: the leaves are still those of the pre-sample's draw)
                    torch.testing.assert_close(L.S["weights"].cpu().double(),
                                               _want_weights(rp, L.S, L.num_q_updates, rt), rtol=1e-5, atol=0)
                    ws.append(L.S["weights"].clone())
                return
            L.steps(4)
            torch.cuda.synchronize()
            ws.extend(w.clone() for w in tr.w)
            for _ in range(n - 4):
                L.step()
                torch.cuda.synchronize()
                ws.append(L.S["weights"].clone())

        run(5)
        assert L.update_index() == L.num_q_updates == 5
        _mutate(rp)
        L._sample()                      # the fresh draw at the head of update 5
        torch.cuda.synchronize()
        fresh = L.S["weights"].clone()
        torch.testing.assert_close(fresh.cpu().double(), _want_weights(rp, L.S, 5, rt), rtol=1e-5, atol=0)
        run(6)
        assert L.update_index() == L.num_q_updates == 11
        out[graphs] = (L.p32.clone(), L.rms_m.clone(), L.rms_v.clone(), L._pbf_all.clone(), rp.ctr.clone(), fresh, ws)
        assert float(L.rms_m.abs().max()) > 0
    a, b = out[True], out[False]
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    assert len(a[6]) == len(b[6]) == 11
    for u, (x, y) in enumerate(zip(a[6], b[6])):
        assert torch.equal(x, y), u


# --------------------------------------------------------- 4. forced DP, world 1
def _forced_dp_worker(q, port):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0")
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.parallel.dist import Comm
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    torch.cuda.set_device(DEV)
    comm = Comm.from_env(device=DEV, force=True)
    out = {}
    for sh in ("off", "on"):
        cfg = _cfg({"use_graphs": True, "presample": True, "force_dp": True, "comm_backend": "native",
                    "dp_fc_exchange": "factors", "dp_shard_update": sh}, q_target_sync_freq=1000)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=0x5EED)
        _fill(rp)
        torch.manual_seed(3)
        L = FusedNatureLearner(cfg, DEV, rp, comm=comm)
        assert L._dp and L._shard == (sh == "on") and L._opt.adam
        L.steps(6)
        torch.cuda.synchronize()
        L.materialize()
        out[sh] = dict(p=L.p32.cpu(), v=L.rms_v.cpu(), m=L.rms_m.cpu(), pb=L._pbf_all.cpu(), leaf=rp.leaf.cpu(),
                       w=L.S["weights"].cpu(), idx=L.update_index(), graphs=L._graphs_enabled())
    comm.shutdown()
    q.put({"same": {k: bool(torch.equal(out["on"][k], out["off"][k])) for k in ("p", "v", "m", "pb", "leaf", "w")},
           "idx": [out["off"]["idx"], out["on"]["idx"]], "graphs": [out["off"]["graphs"], out["on"]["graphs"]],
           "moved": float(out["on"]["m"].abs().max())})


def test_forced_dp_adam_sharded_update_equals_unsharded():
    import queue
    import random
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_forced_dp_worker, args=(q, 29600 + random.randint(601, 900)))
    p.start()
    res = None
    for _ in range(400):
        try:
            res = q.get(timeout=1)
            break
        except queue.Empty:
            if not p.is_alive():
                break
    p.join(timeout=60)
    assert res is not None and p.exitcode == 0
    assert all(res["same"].values()), res
    assert res["idx"] == [6, 6] and res["graphs"] == [True, True] and res["moved"] > 0, res


# ------------------------------------------------------------------ 5. resume
def test_gpu_adam_resume_matches_uninterrupted_run(tmp_path):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg = _cfg({"use_graphs": True}, q_target_sync_freq=3)
    rp = _replay(seed=5)
    torch.manual_seed(0)
    L = FusedNatureLearner(cfg, DEV, rp)
    for _ in range(4):
        L.step()
    torch.cuda.synchronize()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(5):
        L.step()
    torch.cuda.synchronize()
    rp2 = _replay(seed=5)
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.num_q_updates == L2.update_index() == 4
    for _ in range(5):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.S["weights"], L2.S["weights"])):
        assert torch.equal(a, b)


# --------------------------------------------------------------- 6. refusals
class _Small:
    """n = 4096 parameters, B = 8, a replay of capacity 64; every buffer holds a value an update, a target
    average or a draw would change."""
    n, B = 4096, 8

    def __init__(self):
        from apex_dqn_amd.ops.fused_ops import HipBackend
        from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
        n, B = self.n, self.B
        self.be = HipBackend()
        self.rp = GpuReplayShard(64, 64, 64, 4, device=DEV, seed=7)
        _fill(self.rp, K=48)
        f = lambda x, dt=torch.float32, k=n: torch.full((k,), x, dtype=dt, device=DEV)
        self.p, self.g, self.v, self.m, self.t = f(1.0), f(0.5), f(1e-6), f(1e-4), f(2.0)
        self.hi, self.th = f(0.0, torch.bfloat16), f(0.0, torch.bfloat16)
        self.part, self.gn = f(1.0, torch.float64, 1024), f(-1.0, k=1)
        self.S = self.rp.alloc_sample_buffers(B)
        self.S["idx"].fill_(-1)
        self.nxt2 = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def args(self, p=None):
        return (self.p if p is None else p, self.g, self.v, self.m, self.hi, 1e-4, 0.95, 1.5e-7, 40.0, True,
                self.part, self.gn)

    def form_kw(self, form):
        """The producer-partials launch (``apex_opt_step``) or the fused optimizer + sample launch
        (``apex_opt_sample``); with the partials given, a refused call launches nothing at all."""
        kw = dict(norm_total=(self.part, 1))
        if form == "sample":
            kw["sample"] = (self.rp, self.B, self.S, self.nxt2)
        return kw

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.p == 1.0).all()) and bool((self.v == 1e-6).all()) and bool((self.t == 2.0).all())
                and not self.hi.any() and not self.th.any() and float(self.gn) == -1.0
                and bool((self.S["idx"] == -1).all()) and int(self.rp.ctr.item()) == 0)


@pytest.mark.parametrize("form", ["step", "sample"])
@pytest.mark.parametrize("bad", ["p_misaligned", "adam_no_counter", "rho", "target_misaligned"])
def test_shared_optimizer_refusals_hold_in_both_launch_forms(form, bad):
    """What the launchers' common check (csrc/rmsprop_common.h ``opt_args_ok``) refuses, it refuses in the
    plain and in the fused optimizer + sample form; nothing is launched."""
    s = _Small()
    args, kw = s.args(), s.form_kw(form)
    if bad == "p_misaligned":                  # 4 bytes off the float4 path
        args = s.args(torch.ones(s.n + 1, device=DEV)[1:])
    elif bad == "adam_no_counter":
        kw["opt"] = adam_spec(DEV)
        kw["opt"].ctr = None
    elif bad == "rho":                         # a rate outside [0, 1]
        kw["target"] = (s.t, s.th, None, 1.5, None)
    else:
        kw["target"] = (torch.full((s.n + 1,), 2.0, device=DEV)[1:], s.th, None, 0.25, None)
    with pytest.raises(RuntimeError, match="opt_step" if form == "step" else "opt_sample"):
        s.be.optimizer(*args, **kw)
    assert s.untouched()


def test_each_optimizer_form_keeps_its_own_refusals():
    """``segs`` with a target (the sample form), ``frag_out`` and ``norm_prefix`` outside the fused launch
    (the plain form): refused by the backend, and by the launchers when handed such a block directly."""
    from apex_dqn_amd.ops import _lib
    s = _Small()
    be, n = s.be, s.n
    target = (s.t, s.th, None, 0.25, None)
    fo = _lib.CfFragOut()
    fo.w1frag, fo.c2f, fo.C = s.hi.data_ptr(), s.th.data_ptr(), 1
    with pytest.raises(ValueError, match="sharded"):
        be.optimizer(*s.args(), **s.form_kw("sample"), segs=[(0, n)], target=target)
    with pytest.raises(ValueError, match="frag_out"):
        be.optimizer(*s.args(), **s.form_kw("step"), frag_out=fo)
    with pytest.raises(ValueError, match="norm_prefix"):
        be.optimizer(*s.args(), **s.form_kw("step"), norm_prefix=s.g[:64])
    st = _lib.stream_ptr()

    def block(**kw):
        a = be._opt_args(*s.args()[:10], s.gn, None, None, kw.get("frag_out"), kw.get("norm_prefix"), None,
                         kw.get("target"))
        a.partials, a.npart = s.part.data_ptr(), 1
        return a
    assert be.lib.apex_opt_step(block(frag_out=fo), st) == 1
    assert be.lib.apex_opt_step(block(norm_prefix=s.g[:64]), st) == 1
    sg = _lib.RmsSegs()
    sg.nseg, sg.off[0], sg.len[0] = 1, 0, n
    sa = s.rp.sample_launch_args(s.B, s.S, s.nxt2)
    assert be.lib.apex_opt_sample(block(target=target), sa, ctypes.byref(sg), st) == 1
    assert s.untouched()
    # the same blocks without the offending member run
    assert be.lib.apex_opt_sample(block(), sa, ctypes.byref(sg), st) == 0
    torch.cuda.synchronize()
    assert not s.untouched() and bool((s.S["idx"] >= 0).all())


def test_sharded_draw_of_two_rows_is_refused_by_the_optimizer_form():
    """``shard_stats`` set and B = 2 (a sharded draw needs B >= 3): the fused form's launcher refuses."""
    s = _Small()
    s.rp.enable_sharding(0, 1, 3)
    S2, nxt2 = s.rp.alloc_sample_buffers(2), torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    S2["idx"].fill_(-1)
    with pytest.raises(RuntimeError, match="opt_sample"):
        s.be.optimizer(*s.args(), norm_total=(s.part, 1), sample=(s.rp, 2, S2, nxt2))
    assert s.untouched() and bool((S2["idx"] == -1).all())
