"""Periodic shrink-and-perturb resets, ``Runtime.reset_interval``, on the CPU: the host mirror
(learner/reset.py) by hand, its tables, the config checks, the fused learner on the torch backend against a
twin that has the mirror applied by hand, Adam's restarted step count, checkpoints and the torch learner."""
import os

import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import reset as RS
from apex_dqn_amd.learner import schedules as sch
from apex_dqn_amd.models.flat_params import ALIGN, FlatLayout, nature_segments
from apex_dqn_amd.ops.fused_ops import split_into

ENV = {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "Runtime.reset_interval"
M64 = (1 << 64) - 1
f32 = np.float32


def _cfg(rt, B=4, env=None, **learner):
    return ApexConfig.from_dict({"env_conf": env or ENV, "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"use_graphs": False, **rt}})


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


def _learner(rt, seed=0, **learner):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(seed)
    return FusedNatureLearner(_cfg(rt, **learner), "cpu", _replay())


# ------------------------------------------------------------ 1. the mirror by hand
def _mix64(z):
    """splitmix64's finaliser in Python integers (independent of the numpy one the mirror uses)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _k24(seed, r, i):
    return _mix64(seed ^ _mix64((r * 0x100000001B3 + i) & M64)) >> 40


def test_seed_is_a_stream_of_its_own():
    from apex_dqn_amd.learner.augment import aug_seed
    from apex_dqn_amd.learner.iqn import iqn_seed
    from apex_dqn_amd.learner.noisy import noise_seed
    s = RS.reset_seed(1234)
    assert s == _mix64(1234 ^ int.from_bytes(b"SPRreset", "big")) & ((1 << 63) - 1)
    assert len({s, aug_seed(1234), iqn_seed(1234), noise_seed(1234), 1234}) == 5
    assert RS.reset_seed(1235) != s and 0 <= s < 1 << 63


# (seed_r, r, i) -> the 24-bit integer, worked through the two splitmix64 rounds with Python integers
HAND = {(0x3DB73FD84B2AC4CF, 1, 0): 16183715, (0x3DB73FD84B2AC4CF, 2, 4097): 9620443, (7, 1 << 33, 3_000_001): 5634232}


def test_fresh_values_by_hand():
    bound = RS.fan_in_bound(3136)
    assert bound == f32(1.0 / 56.0)
    for (seed, r, i), k_want in HAND.items():
        k = _k24(seed, r, i)
        assert k == k_want and 0 <= k < 1 << 24
        phi = f32((2 * k + 1 - (1 << 24)) / float(1 << 24) * float(bound))     # exact in fp64, rounded once
        start = i - i % 4
        row = RS.ResetRow(start, start + 8, 8, 8, float(bound), 0.0, 0, 0.0)
        got = RS.fresh_values(seed, r, [row])
        assert got.dtype == f32 and got.size == start + 8 and got[i] == phi and not got[:start].any()
        assert int(RS.u24(seed, r, i)) == k


def test_fresh_values_range_moments_and_streams():
    n, b = 100_000, RS.fan_in_bound(576)
    row = RS.ResetRow(64, 64 + n, n, n, float(b), 0.0, 0, 0.0)
    seed = RS.reset_seed(1234)
    x = RS.fresh_values(seed, 1, [row])[64:].astype(np.float64)
    assert (np.abs(x) < float(b)).all()                       # strictly inside: 2 k + 1 is odd, never +-2^24
    # U(-b, b): mean 0, variance b^2 / 3; standard errors b / sqrt(3 n) and b^2 sqrt(4 / 45) / sqrt(n)
    bb = float(b)
    assert abs(x.mean()) < 4 * bb / np.sqrt(3 * n)
    assert abs(x.var() - bb * bb / 3) < 4 * bb * bb * np.sqrt(4.0 / 45.0 / n)
    again = RS.fresh_values(seed, 1, [row])[64:]
    assert np.array_equal(again.view(np.uint32), x.astype(f32).view(np.uint32))
    for other in (RS.fresh_values(seed, 2, [row]), RS.fresh_values(RS.reset_seed(1235), 1, [row])):
        assert (other[64:] != x.astype(f32)).mean() > 0.99
    # the extreme integers give the extreme values, symmetric and inside the range
    lo = f32((1 - (1 << 24)) / float(1 << 24) * bb)
    assert -bb < lo < 0 and f32((2 * ((1 << 24) - 1) + 1 - (1 << 24)) / float(1 << 24) * bb) == -lo


LAYOUTS = {
    "scalar": (dict(), dict(C=4, A=4)),
    "nature32": (dict(network="nature32"), dict(C=4, A=4)),
    "noisy3": (dict(noisy=True, num_atoms=3, noisy_sigma0=0.4), dict(C=4, A=4, num_atoms=3, noisy=True)),
    "implicit": (dict(num_atoms=8, dist_head="implicit"), dict(C=4, A=4, implicit=True)),
}


def _table(kind, a_e=0.5, a_h=0.0):
    rt, seg = LAYOUTS[kind]
    cfg = _cfg({**rt, "reset_interval": 5, "reset_shrink_encoder": a_e, "reset_shrink_head": a_h},
               env={**ENV, "action_dim": seg["A"]})
    lay = FlatLayout(nature_segments(seg["C"], seg["A"], 64, seg.get("num_atoms", 1), noisy=seg.get("noisy", False),
                                     implicit=seg.get("implicit", False)))
    return lay, cfg, RS.reset_table(lay, cfg)


@pytest.mark.parametrize("kind", list(LAYOUTS))
def test_reset_table(kind):
    lay, cfg, tab = _table(kind, 0.25, 0.75)
    assert len(tab) == len(lay.segments) <= RS.MAX_ROWS
    fan = {"w1": 256, "b1": 256, "w2": 16 * (32 if kind == "nature32" else 64), "w3": 576, "b3": 576, "wfc": 3136,
           "bfc": 3136, "wv": 512, "bv": 512, "wa": 512, "ba": 512, "wtau": 64, "btau": 64}
    fan["b2"] = fan["w2"]
    prev = 0
    for (name, shape), row in zip(lay.segments, tab):
        n = int(np.prod(shape))
        assert row.start == lay.offsets[name] and row.end == row.start + n      # every segment once, gaps excluded
        assert row.start % ALIGN == 0 and row.start >= prev
        prev = row.end
        assert row.alpha == (0.25 if name in ("w1", "b1", "w2", "b2", "w3", "b3") else 0.75), name
        if name.startswith("s"):       # a sigma segment: NoisyLinear's constant of its layer
            p = 3136 if name.endswith("fc") else 512
            assert row.const_flag == 1 and f32(row.const_value) == f32(0.4 / p ** 0.5)
        else:
            assert row.const_flag == 0 and f32(row.bound) == f32(1.0 / np.sqrt(float(fan[name]))), name
    assert prev <= lay.numel
    rows = {name: row for (name, _), row in zip(lay.segments, tab)}
    c1 = 32 if kind == "nature32" else 64
    assert (rows["w1"].period, rows["w1"].live) == (64 * 4 * 64, c1 * 4 * 64)
    assert (rows["b1"].period, rows["b1"].live) == (64, c1) and (rows["w2"].period, rows["w2"].live) == (64, c1)
    assert all(r.live == r.period == r.end - r.start for k, r in rows.items() if k not in ("w1", "b1", "w2"))
    assert ("wtau" in rows) == (kind == "implicit") and ("swfc" in rows) == (kind == "noisy3")
    phi = RS.fresh_values(RS.reset_seed(0), 1, tab)
    V = lay.views(torch.from_numpy(np.concatenate([phi, np.zeros(lay.numel - phi.size, f32)])))
    if kind == "nature32":             # the padding's phi is 0, everything live is drawn
        assert not V["w1"][32:].any() and not V["b1"][32:].any() and not V["w2"][..., 32:].any()
        assert V["w1"][:32].all() and V["b1"][:32].all() and V["w2"][..., :32].all()
    else:
        assert V["w1"].all() and V["w2"].all()
    for a, b in zip(tab, tab[1:]):     # gaps hold no value
        assert not phi[a.end:b.start].any()


def test_check_table_refuses():
    ok = RS.ResetRow(0, 8, 8, 8, 0.1, 0.5, 0, 0.0)
    RS.check_table([ok], 8, align=4)
    for bad, n in (([ok._replace(start=2)], 8), ([ok, ok], 16), ([ok._replace(end=12)], 8),
                   ([ok._replace(live=9)], 8), ([ok._replace(alpha=1.5)], 8), ([], 8),
                   ([ok._replace(start=8 * k, end=8 * k + 8) for k in range(33)], 1024)):
        with pytest.raises(ValueError):
            RS.check_table(bad, n, align=4)


# --------------------------------------------------------------- 2. apply_reset
@pytest.mark.parametrize("kind", ["noisy3", "nature32"])
def test_apply_reset_alphas(kind):
    out = {}
    for alpha in (0.0, 0.5, 1.0):
        lay, cfg, tab = _table(kind, alpha, alpha)
        rng = np.random.default_rng(1)
        p, t, v, m = (rng.normal(size=lay.numel).astype(f32) for _ in range(4))
        if kind == "nature32":         # the padded elements are exact zeros in both nets
            for a in (p, t):
                V = lay.views(torch.from_numpy(a))
                V["w1"][32:] = 0
                V["b1"][32:] = 0
                V["w2"][..., 32:] = 0
        p0, t0, v0, m0 = (a.copy() for a in (p, t, v, m))
        seed = RS.reset_seed(5)
        RS.apply_reset(p, t, v, m, seed, 2, tab)
        phi = RS.fresh_values(seed, 2, tab)
        inside = np.zeros(lay.numel, bool)
        for row in tab:
            inside[row.start:row.end] = True
        assert not v[inside].any() and not m[inside].any()                       # whatever alpha
        for new, old in ((p, p0), (t, t0), (v, v0), (m, m0)):                    # the gaps are not touched
            assert np.array_equal(new[~inside], old[~inside])
        ph = np.concatenate([phi, np.zeros(lay.numel - phi.size, f32)])
        if alpha == 1.0:
            assert np.array_equal(p.view(np.uint32), p0.view(np.uint32)) and np.array_equal(t, t0)
        elif alpha == 0.0:
            assert np.array_equal(p[inside], ph[inside]) and np.array_equal(t[inside], ph[inside])
            if kind == "noisy3":       # a fully reset sigma segment is what the module's constructor writes
                from apex_dqn_amd.models.dueling import NoisyLinear
                V = lay.views(torch.from_numpy(p))
                assert torch.equal(V["swfc"][:512], NoisyLinear(3136, 512, 0.4).weight_sigma)
                assert torch.equal(V["sba"], NoisyLinear(512, 12, 0.4).bias_sigma)
        else:
            a = f32(0.5)
            want = (a * p0).astype(f32) + (a * ph).astype(f32)
            assert np.array_equal(p[inside], want.astype(f32)[inside])
            # the online - target gap is scaled by alpha, up to the two sums' roundings
            gap = np.abs((p - t).astype(np.float64) - 0.5 * (p0.astype(np.float64) - t0))
            assert (gap[inside] <= 2.0 ** -23 * (np.abs(p) + np.abs(t))[inside]).all()
        if kind == "nature32":
            V = lay.views(torch.from_numpy(p))
            assert not V["w1"][32:].any() and not V["b1"][32:].any() and not V["w2"][..., 32:].any()
        out[alpha] = p
    assert not np.array_equal(out[0.0], out[0.5])
    with pytest.raises(TypeError):
        RS.apply_reset(p.astype(np.float64), t, v, m, 1, 1, tab)


def test_apply_reset_rounds_three_times():
    """fl(fl(a p) + fl(fl(1 - a) phi)): not one fused multiply-add and not p + (1 - a)(phi - p)."""
    n = 4096
    row = RS.ResetRow(0, n, n, n, float(RS.fan_in_bound(64)), 0.3, 0, 0.0)
    rng = np.random.default_rng(0)
    p0 = rng.normal(size=n).astype(f32)
    p, t, v, m = p0.copy(), p0.copy(), np.ones(n, f32), np.ones(n, f32)
    RS.apply_reset(p, t, v, m, 9, 1, [row])
    phi = RS.fresh_values(9, 1, [row])
    a = f32(0.3)
    b = f32(f32(1.0) - a)
    want = np.array([f32(f32(a * x) + f32(b * y)) for x, y in zip(p0, phi)], f32)
    assert np.array_equal(p, want) and np.array_equal(t, p)
    fused = (a.astype(np.float64) * p0 + (b * phi).astype(f32)).astype(f32)
    assert not np.array_equal(p, fused) and not np.array_equal(p, (p0 + b * (phi - p0)).astype(f32))


# -------------------------------------------------------------------- 3. config
def test_config_defaults_round_trip_and_bundled_config():
    rt = ApexConfig.from_dict({}).Runtime
    assert (rt.reset_interval, rt.reset_shrink_encoder, rt.reset_shrink_head) == (0, 0.5, 0.0)
    cfg = ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"reset_interval": 7, "reset_shrink_encoder": 0.25,
                                                             "reset_shrink_head": 1}})
    rt = ApexConfig.from_dict(cfg.to_dict()).Runtime
    assert (rt.reset_interval, rt.reset_shrink_encoder, rt.reset_shrink_head) == (7, 0.25, 1)
    b = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_reset.json"))
    d = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_drq.json"))
    assert b.Runtime.reset_interval == 40000 and b.Runtime.reset_shrink_encoder == 0.5 \
        and b.Runtime.reset_shrink_head == 0.0 and b.Runtime.optimizer == "adam" and b.Runtime.target_ema_rate > 0 \
        and b.Runtime.augment_shift == d.Runtime.augment_shift >= 1


@pytest.mark.parametrize("rt,key", [
    ({"reset_interval": -1}, KEY), ({"reset_interval": 2.5}, KEY), ({"reset_interval": True}, KEY),
    ({"reset_interval": "3"}, KEY),
    ({"reset_shrink_encoder": -0.1}, "Runtime.reset_shrink_encoder"),
    ({"reset_shrink_encoder": 1.5}, "Runtime.reset_shrink_encoder"),
    ({"reset_shrink_encoder": True}, "Runtime.reset_shrink_encoder"),
    ({"reset_shrink_head": float("nan")}, "Runtime.reset_shrink_head"),
    ({"reset_shrink_head": "0"}, "Runtime.reset_shrink_head"), ({"reset_shrink_head": 2}, "Runtime.reset_shrink_head"),
    ({"reset_interval": 5, "network": "impala"}, KEY), ({"reset_interval": 5, "world_size": 2}, KEY),
    ({"reset_interval": 5, "force_dp": True}, KEY)])
def test_config_refusals_name_the_key(rt, key):
    with pytest.raises(ValueError, match=key):
        ApexConfig.from_dict({"env_conf": ENV, "Runtime": rt})


def test_config_accepts_the_range_ends():
    for ok in ({"reset_interval": 0}, {"reset_interval": 1, "reset_shrink_encoder": 0, "reset_shrink_head": 1},
               {"reset_interval": 10 ** 9, "reset_shrink_encoder": 1.0, "reset_shrink_head": 0.0}):
        ApexConfig.from_dict({"env_conf": ENV, "Runtime": ok})


def test_learners_refuse_the_data_parallel_step_and_the_graph_learner():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    from apex_dqn_amd.learner.impala_learner import FusedImpalaLearner
    from apex_dqn_amd.parallel.dist import EmulatedComm
    cfg = _cfg({"reset_interval": 5})
    with pytest.raises(ValueError, match=KEY):      # the emulated world
        FusedNatureLearner(cfg, "cpu", _replay(), comm=EmulatedComm(8, 0, torch.device("cpu")))
    with pytest.raises(ValueError, match=KEY):
        GraphLearner(cfg, "cpu", _replay())
    imp = _cfg({"network": "impala"})
    imp.Runtime.reset_interval = 5                  # (past the config check)
    with pytest.raises(ValueError, match=KEY):
        FusedImpalaLearner(imp, "cpu", _replay())


# ------------------------------------------- 4. fused learner, torch backend, vs a twin
ADAM = {"optimizer": "adam", "lr": 2.5e-4, "lr_warmup_steps": 2}
HEADS = {"scalar": {}, "qr_noisy": {"num_atoms": 5, "dist_head": "quantile", "noisy": True},
         "implicit": {"num_atoms": 4, "dist_head": "implicit"}}
STATE = ("p32", "t32", "rms_v", "rms_m", "pbf", "tbf", "td_abs")


def _hand_reset(L, r, I, cfg):
    """The mirror on a learner that runs without the key: parameters, target and moments in place, then every
    derived format as ``load`` refreshes them, and Adam's reset word."""
    tab = RS.reset_table(L.layout, cfg)
    RS.apply_reset(L.p32.numpy(), L.t32.numpy(), L.rms_v.numpy(), L.rms_m.numpy(), RS.reset_seed(cfg.Runtime.seed), r, tab)
    split_into(L.p32, L.pbf, L.pbf_lo)
    split_into(L.t32, L.tbf, L.tbf_lo)
    L._online_changed()
    L._target_changed()
    if L._opt is not None and L._opt.adam:
        L._opt.t0 = torch.tensor([r * I], dtype=torch.int64)


# optimizer x target x head in full; pre-sampling (it only moves the next batch's draw into the optimizer call, ahead
# of the reset instead of behind it) alternates over them, so every optimizer, target and head meets both settings
CASES = [(o, t, h, (i + j + k) % 2 == 0) for i, o in enumerate(("rmsprop", "adam")) for j, t in enumerate(("hard", "ema"))
         for k, h in enumerate(HEADS)]


@pytest.mark.parametrize("opt,target,head,presample", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_fused_learner_equals_twin_with_the_mirror_by_hand(opt, target, head, presample):
    I = 3
    rt = {**HEADS[head], **(ADAM if opt == "adam" else {}), "presample": presample, "seed": 11,
          **({"target_ema_rate": 0.1} if target == "ema" else {})}
    A = _learner({**rt, "reset_interval": I}, q_target_sync_freq=3)
    B = _learner(rt, q_target_sync_freq=3)
    cfg = A.cfg
    assert A.reset_I == I and B.reset_I == 0 and B.upd_t0 is None
    assert (A.upd_t0 is not None and A._opt.t0 is A.upd_t0) if opt == "adam" else (A._opt is None or A._opt.t0 is None)
    for u in range(1, 8):
        A.step()
        B.step()
        if u % I == 0:
            before = B.p32.clone()
            _hand_reset(B, u // I, I, cfg)
            assert not torch.equal(before, B.p32) and not B.rms_v.any() and not B.rms_m.any()
            assert int(A.upd_t0) == u
            if target == "hard":       # the coinciding sync ran first: a fully reset head has target = online
                assert torch.equal(A.T["wfc"], A.P["wfc"]) and torch.equal(A.t32, A.p32)
            else:
                assert torch.equal(A.T["wfc"], A.P["wfc"]) and not torch.equal(A.T["w3"], A.P["w3"])
        for name in STATE:
            assert torch.equal(getattr(A, name), getattr(B, name)), (u, name)
    assert A.last_metrics()["resets"] == 2 and "resets" not in B.last_metrics()
    assert A.update_index() == 7 and int(A.upd_t0) == 6


def test_split_planes_follow_the_reset():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(0)
    L = FusedNatureLearner(_cfg({"reset_interval": 2}), "cpu", _replay(), split=True)
    L.step()
    p1 = L.p32.clone()
    L.step()
    assert not torch.equal(p1, L.p32)
    for src, hi_, lo_ in ((L.p32, L.pbf, L.pbf_lo), (L.t32, L.tbf, L.tbf_lo)):
        hi, lo = torch.zeros_like(hi_), torch.zeros_like(lo_)
        split_into(src, hi, lo)
        assert torch.equal(hi, hi_) and torch.equal(lo, lo_)


def test_replay_is_untouched_by_a_reset():
    L = _learner({"reset_interval": 2, "presample": True})
    L.step()
    rp = L.replay
    before = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr, L.S["idx"])]
    L.reset_now(1)
    for a, b in zip(before, (rp.leaf, rp.nodes, rp.min_bits, rp.ctr, L.S["idx"])):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="reset_interval"):
        _learner({}).reset_now(1)


# ------------------------------------------------------------- 5. a reset that never fires
@pytest.mark.parametrize("rt", [{}, ADAM], ids=["rmsprop", "adam"])
def test_interval_beyond_the_run_changes_nothing(rt):
    A = _learner({**rt, "reset_interval": 1000})
    B = _learner(rt)
    for u in range(3):
        A.step()
        B.step()
        for name in STATE:
            assert torch.equal(getattr(A, name), getattr(B, name)), (u, name)
    assert A.last_metrics()["resets"] == 0


def test_default_passes_no_reset_word_to_the_backend():
    L = _learner(ADAM)
    assert L.upd_t0 is None and L._opt.t0 is None and not hasattr(L, "_reset_table")
    R = _learner({"reset_interval": 4})           # RMSprop needs no word: zeroed moments are its first state
    assert R._opt is None and hasattr(R, "_reset_table")


# ----------------------------------------------------------- 6. Adam after a reset
def test_adam_after_a_reset_vs_a_fresh_torch_optim_adam():
    """Four updates, a reset, three more: the parameters follow a freshly constructed fp64 ``torch.optim.Adam`` on
    the reset parameters (step count from 1, zero moments) at tests/test_opt_schedules_cpu.py's tolerances; with
    the word left at 0 they do not (the corrections of t = 5.. on zeroed moments under-correct)."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    n, lr, b1, b2, eps, clip = 50_001, 2.5e-4, 0.9, 0.999, 1.5e-4, 40.0
    g = torch.Generator(device="cpu").manual_seed(1)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.01 for _ in range(7)]
    row = RS.ResetRow(0, n - 1, n - 1, n - 1, float(RS.fan_in_bound(64)), 0.5, 0, 0.0)
    be = TorchBackend()
    out = {}
    for with_t0 in (True, False):
        ctr, base = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
        t0 = torch.zeros(1, dtype=torch.int64)
        spec = sch.OptSpec("adam", ctr, base, lr, 2, 3, 2.5e-5, b1, b2, eps, t0=t0)
        p, t, v, m = p0.clone(), p0.clone(), torch.zeros(n), torch.zeros(n)
        pbf, tbf, norm = torch.zeros(n), torch.zeros(n), torch.zeros(1)
        for u, gr in enumerate(grads):
            if u == 4:
                be.reset_perturb([row], 3, 1, p, t, v, m, (pbf, None), (tbf, None))
                assert not v[:-1].any() and not m[:-1].any() and torch.equal(pbf, p) and torch.equal(tbf[:-1], t[:-1]) \
                    and tbf[-1] == 0
                if with_t0:
                    t0.fill_(4)
                tp = torch.nn.Parameter(p.double().clone())
                ref = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps)
            ctr += 1
            be.optimizer(p, gr, v, m, pbf, lr, 0.95, 1.5e-7, clip, True, None, norm, opt=spec)
            if u >= 4:
                tp.grad = gr.double().clone()
                torch.nn.utils.clip_grad_norm_([tp], clip)
                for grp in ref.param_groups:
                    grp["lr"] = float(sch.lr_at(u, lr, 2, 3, 2.5e-5))     # the schedules keep reading u
                ref.step()
        out[with_t0] = (p[:-1], tp.detach().float()[:-1])
    torch.testing.assert_close(*out[True], rtol=1e-5, atol=1e-6)
    assert not torch.allclose(*out[False], rtol=1e-5, atol=1e-6)
    c = sch.adam_corrections(4, b1, b2, t0=4)
    assert c == sch.adam_corrections(0, b1, b2) and c[0] == f32(1 - 0.9)
    assert sch.adam_corrections(9, b1, b2, t0=0) == sch.adam_corrections(9, b1, b2)


# ---------------------------------------------------------------- 7. checkpoints
def test_resume_across_a_boundary_and_load_across_the_setting(tmp_path):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg = _cfg({**ADAM, "reset_interval": 3}, q_target_sync_freq=1000)
    torch.manual_seed(0)
    rp = _replay()
    L = FusedNatureLearner(cfg, "cpu", rp)
    for _ in range(4):
        L.step()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    saved = torch.load(ck, weights_only=True)
    plain = FusedNatureLearner(_cfg(ADAM, q_target_sync_freq=1000), "cpu", _replay())
    ck0 = str(tmp_path / "plain.pt")
    plain.save(ck0)
    assert set(saved) == set(torch.load(ck0, weights_only=True))         # a checkpoint gains no keys
    assert saved["config"]["Runtime"]["reset_interval"] == 3
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    p_saved = L.p32.clone()
    for _ in range(3):
        L.step()
    rp2 = _replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), "cpu", rp2)
    assert L2.num_q_updates == 4 and int(L2.upd_t0) == 3
    for _ in range(3):
        L2.step()
    assert int(L2.upd_t0) == 6 and L2.last_metrics()["resets"] == 2
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (L.tbf, L2.tbf),
                 (rp.leaf, rp2.leaf), (L.td_abs, L2.td_abs)):
        assert torch.equal(a, b)
    # across the setting, both ways
    assert plain.load(ck) and torch.equal(plain.p32, p_saved) and plain.upd_t0 is None
    plain.step()
    R = FusedNatureLearner(cfg, "cpu", _replay())
    assert R.load(ck0) and R.num_q_updates == 0 and int(R.upd_t0) == 0
    R.step()


# ------------------------------------------------------------ 8. the torch learner
def test_mlp_torch_learner_follows_the_mirror():
    from apex_dqn_amd.learner.torch_learner import TorchLearner
    over = ["Runtime.reset_interval=2", "Runtime.noisy=true", "Runtime.optimizer=adam", "Learner.q_target_sync_freq=1000"]
    cfg = ApexConfig.load(os.path.join(ROOT, "configs", "cartpole.json"), over)
    cfg0 = ApexConfig.load(os.path.join(ROOT, "configs", "cartpole.json"), over[1:])
    torch.manual_seed(0)
    A = TorchLearner(cfg, "cpu")
    torch.manual_seed(0)
    B = TorchLearner(cfg0, "cpu")
    rng = np.random.default_rng(0)
    batch = dict(S_t=rng.normal(size=(8, 4)).astype(f32), S_tpn=rng.normal(size=(8, 4)).astype(f32),
                 A_t=rng.integers(0, 2, 8), R=rng.normal(size=8).astype(f32),
                 Gamma=np.full(8, 0.9, f32), weights=np.ones(8, f32))
    tab = RS.module_reset_table(A.Q, cfg)
    names = [k for k, _ in A.Q.named_parameters()]
    assert [r.end - r.start for r in tab] == [p.numel() for p in A.Q.parameters()] and tab[0].start == 0
    rows = dict(zip(names, tab))
    assert rows["layer1.0.weight"].alpha == 0.5 and rows["value.bias"].alpha == 0.0
    assert f32(rows["layer1.0.bias"].bound) == f32(0.5)                   # fan-in 4, its weight's
    assert rows["value.weight_sigma"].const_flag == 1 and rows["value.bias_sigma"].const_flag == 1
    for u in range(1, 5):
        outA = A.step(batch)
        B.step(batch)
        if u % 2 == 0:     # the twin: the mirror by hand on the flat concatenation, a fresh optimizer
            from apex_dqn_amd.learner.torch_learner import make_optimizer
            flat = [np.concatenate([x.detach().numpy().ravel() for x in net.parameters()]) for net in (B.Q, B.Q_target)]
            z = np.zeros_like(flat[0])
            RS.apply_reset(flat[0], flat[1], z, z.copy(), RS.reset_seed(cfg.Runtime.seed), u // 2, tab)
            with torch.no_grad():
                for net, a in zip((B.Q, B.Q_target), flat):
                    for row, x in zip(tab, net.parameters()):
                        x.copy_(torch.from_numpy(a[row.start:row.end]).reshape(x.shape))
            B.optimizer = make_optimizer(B.Q.parameters(), B.rt)
            assert torch.equal(A.Q.value.weight, A.Q_target.value.weight)          # alpha_h = 0
            assert torch.equal(A.Q.value.weight_sigma, torch.full_like(A.Q.value.weight_sigma, 0.5 / A.Q.value.in_features ** 0.5))
        for a, b in zip(list(A.Q.parameters()) + list(A.Q_target.parameters()),
                        list(B.Q.parameters()) + list(B.Q_target.parameters())):
            assert torch.equal(a, b), u
        assert outA["resets"] == u // 2 and np.isfinite(outA["loss"])


def test_inline_cartpole_runs_with_resets():
    from apex_dqn_amd.runtime.loops import train_inline
    cfg = ApexConfig.load(os.path.join(ROOT, "configs", "cartpole.json"), ["Runtime.reset_interval=50"])
    assert cfg.Runtime.reset_interval == 50 and cfg.network == "mlp"
    out = train_inline(cfg, 120)
    T = out["learner"]
    assert T.num_q_updates == 120 and len(out["losses"]) == 120 and np.isfinite(out["losses"]).all()
    assert T.last_metrics()["resets"] == 2
