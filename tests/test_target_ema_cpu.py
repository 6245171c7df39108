"""The soft (Polyak) target network, ``Runtime.target_ema_rate``, on the CPU: config checks, the
host mirror (learner/schedules.py ``target_ema``), the fused learner on the torch backend against
the mirror, the heads that read the averaged target, checkpoints and the torch learner."""
import os

import numpy as np
import pytest
import torch

from apex_dqn_amd.config import ApexConfig
from apex_dqn_amd.learner import schedules as sch
from apex_dqn_amd.ops.fused_ops import split_into

ENV = {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "Runtime.target_ema_rate"


def _cfg(rt, B=8, **learner):
    return ApexConfig.from_dict({"env_conf": ENV, "Learner": {"replay_sample_size": B, **learner},
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


# ------------------------------------------------------------------ 1. config
def test_config_default_round_trip_and_bundled_config():
    cfg = ApexConfig.from_dict({})
    assert cfg.Runtime.target_ema_rate == 0.0
    cfg = ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"target_ema_rate": 0.25}})
    assert ApexConfig.from_dict(cfg.to_dict()).Runtime.target_ema_rate == 0.25
    for ok in (0, 1, 0.0, 1.0, 0.005):
        ApexConfig.from_dict({"env_conf": ENV, "Runtime": {"target_ema_rate": ok}})
    b = ApexConfig.load(os.path.join(ROOT, "configs", "pong_1gpu_ema.json"))
    assert b.Runtime.target_ema_rate == 0.005 and b.Runtime.noisy and b.Runtime.num_atoms == 51 \
        and b.Runtime.optimizer == "adam"


@pytest.mark.parametrize("rt", [{"target_ema_rate": -0.01}, {"target_ema_rate": 1.5}, {"target_ema_rate": True},
                                {"target_ema_rate": False}, {"target_ema_rate": "0.5"},
                                {"target_ema_rate": float("nan")},
                                {"target_ema_rate": 0.1, "network": "impala"},
                                {"target_ema_rate": 0.1, "world_size": 2},
                                {"target_ema_rate": 0.1, "force_dp": True}])
def test_config_refusals_name_the_key(rt):
    with pytest.raises(ValueError, match=KEY):
        ApexConfig.from_dict({"env_conf": ENV, "Runtime": rt})


def test_learners_refuse_the_data_parallel_step_and_the_graph_learner():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.learner.graph_learner import GraphLearner
    from apex_dqn_amd.learner.impala_learner import FusedImpalaLearner
    from apex_dqn_amd.parallel.dist import EmulatedComm
    cfg = _cfg({"target_ema_rate": 0.1})
    with pytest.raises(ValueError, match=KEY):      # the emulated world
        FusedNatureLearner(cfg, "cpu", _replay(), comm=EmulatedComm(8, 0, torch.device("cpu")))
    with pytest.raises(ValueError, match=KEY):
        GraphLearner(cfg, "cpu", _replay())
    imp = _cfg({"network": "impala"})
    imp.Runtime.target_ema_rate = 0.1               # (past the config check)
    with pytest.raises(ValueError, match=KEY):
        FusedImpalaLearner(imp, "cpu", _replay())


# ------------------------------------------------------------------ 2. mirror
def test_mirror_by_hand():
    f32 = np.float32
    t = np.array([1.0, -3.0, 0.1, 1e-8], f32)
    p = np.array([2.0, 5.0, 0.3, -7.25], f32)
    one = sch.target_ema(t, p, 1.0)
    assert one.dtype == f32 and np.array_equal(one, p)
    half = sch.target_ema(t, p, 0.5)               # halving is exact: (t + p) / 2 rounded once
    assert np.array_equal(half, (t * f32(0.5) + p * f32(0.5)).astype(f32))
    assert half[0] == f32(1.5) and half[1] == f32(1.0)
    r = f32(0.3)
    a = f32(f32(1.0) - r)
    want = np.array([f32(f32(a * x) + f32(r * y)) for x, y in zip(t, p)], f32)
    assert np.array_equal(sch.target_ema(t, p, 0.3), want)
    # not t + r (p - t), and not one fused multiply-add: some element of a random vector differs
    rng = np.random.default_rng(0)
    t, p = rng.normal(size=4096).astype(f32), rng.normal(size=4096).astype(f32)
    m = sch.target_ema(t, p, 0.3)
    assert not np.array_equal(m, (t + r * (p - t)).astype(f32))
    fused = (a.astype(np.float64) * t + (r * p).astype(f32)).astype(f32)      # fma(a, t, fl(r p))
    assert not np.array_equal(m, fused)
    assert np.array_equal(sch.target_ema(t, p, 0.0), t)
    with pytest.raises(TypeError):
        sch.target_ema(t.astype(np.float64), p, 0.5)


# ------------------------------------------------- 3. fused learner, torch backend
@pytest.mark.parametrize("presample", [False, True])
def test_fused_learner_follows_the_mirror(presample):
    L = _learner({"target_ema_rate": 0.25, "presample": presample}, q_target_sync_freq=2)
    assert L.ema == 0.25 and torch.equal(L.t32, L.p32)              # the target starts as a copy
    for u in range(4):
        t0 = L.t32.numpy().copy()
        L.step()
        want = sch.target_ema(t0, L.p32.numpy(), 0.25)
        assert np.array_equal(L.t32.numpy(), want), u
        hi = torch.zeros_like(L.tbf)
        split_into(L.t32, hi, None)
        assert torch.equal(L.tbf, hi) and L.tbf_lo is None
        if u == 1:
            assert not torch.equal(L.t32, L.p32)                    # the hard sync is off
    m = L.last_metrics()
    assert m["target_gap"] == float((L.P["wfc"] - L.T["wfc"]).abs().mean()) and m["target_gap"] > 0


def test_split_planes_follow_the_target():
    """The torch backend emulating the split (hi / lo) operands: both planes are the project's split of t32."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    torch.manual_seed(0)
    L = FusedNatureLearner(_cfg({"target_ema_rate": 0.25}), "cpu", _replay(), split=True)
    for _ in range(2):
        t0 = L.t32.numpy().copy()
        L.step()
        assert np.array_equal(L.t32.numpy(), sch.target_ema(t0, L.p32.numpy(), 0.25))
        hi, lo = torch.zeros_like(L.tbf), torch.zeros_like(L.tbf_lo)
        split_into(L.t32, hi, lo)
        assert torch.equal(L.tbf, hi) and torch.equal(L.tbf_lo, lo)


def test_rate_one_equals_hard_sync_every_update():
    A = _learner({"target_ema_rate": 1.0}, q_target_sync_freq=1000)
    B = _learner({}, q_target_sync_freq=1)
    for u in range(3):
        A.step()
        B.step()
        for name in ("td_abs", "p32", "rms_v", "rms_m", "t32"):
            assert torch.equal(getattr(A, name), getattr(B, name)), (u, name)
    assert "target_gap" not in B.last_metrics()


def test_default_passes_no_target_to_the_backend():
    seen = {}
    for rho in (0.0, 0.25):
        L = _learner({"target_ema_rate": rho})
        orig, calls = L.ops.optimizer, []

        def spy(*a, _orig=orig, _calls=calls, **k):
            _calls.append(dict(k))
            return _orig(*a, **k)

        L.ops.optimizer = spy
        L.step()
        seen[rho] = calls
    assert len(seen[0.0]) == 1 and "target" not in seen[0.0][0]
    t32, tbf, tbf_lo, rho, tfo = seen[0.25][0]["target"]
    assert rho == 0.25 and tfo is None and tbf_lo is None and t32.dtype == torch.float32


# ----------------------------------- 4. the heads read the averaged target (2 updates)
@pytest.mark.parametrize("rt", [{"num_atoms": 11, "noisy": True}, {"num_atoms": 8, "dist_head": "implicit"},
                                {"munchausen": True}], ids=["c51_noisy", "iqn", "munchausen"])
def test_update_two_reads_the_averaged_target(rt):
    rho = 0.25
    A = _learner({**rt, "target_ema_rate": rho}, q_target_sync_freq=1000)
    B = _learner(rt, q_target_sync_freq=1000)
    t0 = B.t32.numpy().copy()
    A.step()
    B.step()
    assert torch.equal(A.p32, B.p32) and torch.equal(A.td_abs, B.td_abs)
    # B's target set by hand to the mirror's value, in every format its forward reads
    B.t32.copy_(torch.from_numpy(sch.target_ema(t0, B.p32.numpy(), rho)))
    split_into(B.t32, B.tbf, B.tbf_lo)
    B._target_changed()
    assert torch.equal(A.t32, B.t32) and not torch.equal(A.t32, A.p32)
    A.step()
    B.step()
    assert torch.equal(A.td_abs, B.td_abs) and torch.equal(A.p32, B.p32)
    # ... and the target matters to that update: a learner with the stale target differs
    C = _learner(rt, q_target_sync_freq=1000)
    C.step()
    C.step()
    assert not torch.equal(C.td_abs, A.td_abs)


# ---------------------------------------------------------- 5. checkpoints
def test_resume_matches_uninterrupted_run_and_loads_across_the_setting(tmp_path):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    cfg = _cfg({"target_ema_rate": 0.25}, q_target_sync_freq=2)
    torch.manual_seed(0)
    rp = _replay()
    L = FusedNatureLearner(cfg, "cpu", rp)
    for _ in range(2):
        L.step()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    saved = torch.load(ck, weights_only=True)
    assert saved["config"]["Runtime"]["target_ema_rate"] == 0.25
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    t_saved, p_saved = L.t32.clone(), L.p32.clone()
    for _ in range(2):
        L.step()
    rp2 = _replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), "cpu", rp2)
    assert torch.equal(L2.t32, t_saved) and not torch.equal(L2.t32, L2.p32)
    for _ in range(2):
        L2.step()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (L.tbf, L2.tbf),
                 (rp.leaf, rp2.leaf), (L.td_abs, L2.td_abs)):
        assert torch.equal(a, b)
    # across the setting: a hard-sync learner takes the averaged target as saved, and back
    H = FusedNatureLearner(_cfg({}, q_target_sync_freq=1000), "cpu", _replay())
    assert H.load(ck) and torch.equal(H.t32, t_saved) and torch.equal(H.p32, p_saved)
    H.step()
    assert torch.equal(H.t32, t_saved)
    ck2 = str(tmp_path / "hard.pt")
    H.save(ck2)
    E = FusedNatureLearner(cfg, "cpu", _replay())
    assert E.load(ck2) and torch.equal(E.t32, t_saved)
    t0 = E.t32.numpy().copy()
    E.step()
    assert np.array_equal(E.t32.numpy(), sch.target_ema(t0, E.p32.numpy(), 0.25))


# ------------------------------------------------------- 6. the torch learner
def test_torch_learner_on_cartpole_follows_the_mirror():
    from apex_dqn_amd.learner.torch_learner import TorchLearner
    cfg = ApexConfig.load(os.path.join(ROOT, "configs", "cartpole.json"),
                          ["Runtime.target_ema_rate=0.25", "Learner.q_target_sync_freq=2"])
    torch.manual_seed(0)
    L = TorchLearner(cfg, "cpu")
    rng = np.random.default_rng(0)
    batch = dict(S_t=rng.normal(size=(8, 4)).astype(np.float32), S_tpn=rng.normal(size=(8, 4)).astype(np.float32),
                 A_t=rng.integers(0, 2, 8), R=rng.normal(size=8).astype(np.float32),
                 Gamma=np.full(8, 0.9, np.float32), weights=np.ones(8, np.float32))
    for a, b in zip(L.Q.parameters(), L.Q_target.parameters()):
        assert torch.equal(a, b)
    for u in range(4):
        t0 = [t.detach().numpy().copy() for t in L.Q_target.parameters()]
        L.step(batch)
        for old, t, p in zip(t0, L.Q_target.parameters(), L.Q.parameters()):
            assert np.array_equal(t.detach().numpy(), sch.target_ema(old, p.detach().numpy(), 0.25)), u
        assert not all(torch.equal(a, b) for a, b in zip(L.Q.parameters(), L.Q_target.parameters()))
