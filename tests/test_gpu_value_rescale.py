"""Invertible value rescaling of the n-step target (``Runtime.value_rescale``) on the GPU: the device function
of csrc/value_rescale.h through its probe, the RESCALE instantiations of the four loss heads against the fp64
oracles (the scalar head's: tests/ddqn_fixtures.py fed the rescaled target, settled on the CPU by
tests/test_value_rescale_cpu.py; the distributional heads': the torch backend in fp64 with the key, on the
fixtures and at the tolerances of those heads' own files), the whole step against the torch backend, graph
against eager, resume, and the GPU loop on unclipped rewards."""
import numpy as np
import pytest
import torch

import ddqn_fixtures as F
import iqn_fixtures as FI
import test_gpu_c51 as C51
import test_gpu_ddqn_head as D
import test_gpu_iqn as IQ
import test_gpu_qr as QR
import test_value_rescale_cpu as CPU
from apex_dqn_amd.learner import rescale as RS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EPS = 1e-3
EPS32 = float(np.float32(EPS))      # what the launchers hand to the kernels


def _hip(eps=EPS):
    """A HIP backend whose scalar head runs with the key on (the helpers of tests/test_gpu_ddqn_head.py call
    ``be.head`` without it)."""
    from apex_dqn_amd.ops.fused_ops import HipBackend

    class RescaleHip(HipBackend):
        def head(self, *a, **kw):
            return super().head(*a, rescale_eps=eps, **kw)
    return RescaleHip()


@pytest.fixture
def rescaled(monkeypatch):
    """Both backends' distributional heads with ``rescale_eps`` = EPS injected, so that the runners and oracles of
    those heads' own test files (which do not know the keyword) run the rescaled variant."""
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend
    for cls in (TorchBackend, HipBackend):
        for name in ("qr_head", "iqn_head", "c51_head"):
            orig = getattr(cls, name)
            monkeypatch.setattr(cls, name, lambda self, *a, _o=orig, **kw: _o(self, *a, rescale_eps=EPS, **kw))


# ------------------------------------------------------------------ 1. probe
@pytest.mark.parametrize("eps", [1e-3, 1e-2])
def test_probe_within_one_ulp_of_the_mirror(eps):
    """4,099 elements (not a block multiple), y in +-[0, 1e3], R in +-[0, 1e4], Gamma in {0, 0.97, 1}.  The
    kernel rounds an fp64 result to fp32 once: half an fp32 ulp, plus the fp64 evaluation's own last bits (the
    device's sqrt / division and a contracted multiply-add against numpy's), which can move a value that sits
    on a rounding boundary to the neighbouring fp32 number: 1 ulp of the fp32-rounded mirror value."""
    n = 4099
    rng = np.random.default_rng(3)
    mag = lambda hi: np.concatenate([[0.0, hi, 1e-3, 1.0], 10.0 ** rng.uniform(-6, np.log10(hi), n - 4)])     # noqa: E731
    y = (mag(1e3) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    R = (rng.permutation(mag(1e4)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    G = rng.choice(np.array([0.0, 0.97, 1.0], np.float32), n)
    y[:3], R[:3], G[:3] = 0.0, [0.0, 5.0, -5.0], [1.0, 0.0, 0.97]
    be = _hip()
    out = torch.full((n + 61,), -7.0, device=DEV)
    dev = lambda a: torch.from_numpy(a).to(DEV)                           # noqa: E731
    be.value_rescale_probe(dev(y), dev(R), dev(G), eps, out[:n])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == -7.0)                                        # nothing past n
    e32 = float(np.float32(eps))
    ref = RS.rescale_target(R.astype(np.float64), G.astype(np.float64), y.astype(np.float64), e32)
    ref32 = ref.astype(np.float32)
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    err = np.abs(got[:n].astype(np.float64) - ref32.astype(np.float64))
    print(f"probe eps {eps}: {int((err > 0).sum())} of {n} differ from the rounded mirror, worst {float((err / ulp).max()):.2f} ulp")
    assert np.all(np.isfinite(got[:n])) and np.all(err <= ulp), float((err / ulp).max())
    assert got[0] == 0.0 and got[1] == np.float32(RS.h(5.0, e32)) and got[2] == np.float32(RS.h(-5.0, e32))
    for bad in (0.0, 1.5):                                               # eps outside (0, 1] never reaches a launch
        with pytest.raises(ValueError, match="value_rescale_eps"):
            be.value_rescale_probe(dev(y), dev(R), dev(G), bad, out[:n])


# ------------------------------------------------------------------ 2. scalar head
def _scalar_run(B, A, split, case, be=None, **kw):
    r = CPU.rescaled_head_oracle(B, A, split, case)
    fx = F.fixture(B, A, 512, split, CPU.RESCALE_SEED[(B, A)])
    h = D._head_launch(be or _hip(), D._dev(fx["Hon"]), D._dev(fx["Htg"]), D._dev(fx["Hon_lo"]), D._dev(fx["Htg_lo"]),
                       r["inputs"], B, A, 512, **kw)
    return h, r


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", CPU.GPU_HEAD_CASES)
@pytest.mark.parametrize("B,A", CPU.GPU_HEAD_PROBLEMS)
def test_scalar_head_vs_fp64_oracle(B, A, case, split):
    """Both sides of the MAXA switch (A = 4 / 18) and A = 1, bf16 and split, at the tolerances of
    tests/test_gpu_ddqn_head.py; no row is excluded (tests/test_value_rescale_cpu.py test_gpu_fixture_conditions)."""
    h, r = _scalar_run(B, A, split, case)
    D._compare(h, r, split, f"rescaled {case} ({B}, {A})")
    assert bool((h["zeroed"] == 0).all())
    if case == "zero_q":
        assert bool((h["q"] == 0).all())
        want = torch.from_numpy(RS.h(r["inputs"]["rew"].double().numpy(), EPS32)).float().abs()
        torch.testing.assert_close(h["td"], want, rtol=2.0 ** -23, atol=0)      # |h(R) - 0|: the probe's one ulp
    if case == "big_rewards":
        # rewards of several hundred are targets of a few tens: squashed, not clipped
        assert 5 < float(r["T"].abs().max()) < 40 and float(r["inputs"]["rew"].abs().max()) > 100
    # and the plain head on the same inputs gives another answer: the variant is really the one that ran
    from apex_dqn_amd.ops.fused_ops import HipBackend
    fx = F.fixture(B, A, 512, split, CPU.RESCALE_SEED[(B, A)])
    h0 = D._head_launch(HipBackend(), D._dev(fx["Hon"]), D._dev(fx["Htg"]), D._dev(fx["Hon_lo"]), D._dev(fx["Htg_lo"]),
                        r["inputs"], B, A, 512)
    assert not torch.equal(h0["td"], h["td"]) and torch.equal(h0["q"], h["q"])


def test_scalar_head_is_norm():
    B, A = 33, 4
    fx = F.fixture(B, A, 512, False, CPU.RESCALE_SEED[(B, A)])
    isn = D._isn(1.7)
    h, r = _scalar_run(B, A, False, "plain", isn=isn)
    D._compare(h, r, False, "rescaled + IsNorm")
    assert float(isn[1]) == float(fx["isw"].max().double()) / float(np.float64(np.float32(1.7)))
    assert int(isn[2]) == 5 + int((fx["isw"] > 0).sum())


@pytest.mark.parametrize("split", [False, True])
def test_scalar_head_with_the_fc_epilogue_inside_the_launch(split):
    """nz = 3 partial planes, M = 15 rows: the h rows the deferred launch writes are the two-launch path's bit
    for bit, and so is every head output; both against the oracle fed the rescaled target."""
    B, HS, K = 5, 512, 3136
    ha, ha_lo, oa, nz, _ = D._fc_run(B, HS, K, split, 3, True, be=_hip())
    hb, hb_lo, ob, _, _ = D._fc_run(B, HS, K, split, 3, False, be=_hip())
    assert nz == 3
    assert torch.equal(ha[:B], hb[:B]) and bool((ha[B:] == 5.0).all())
    if split:
        assert torch.equal(ha_lo[:B], hb_lo[:B])
    for k in ("td", "loss", "dhead", "q", "dH_hi", "dH"):
        assert torch.equal(oa[k], ob[k]), k
    hbj = F.join64(hb, hb_lo)
    f = F.fc_fixture(B, HS, K, split)
    r0 = F.fc_head_oracle(B, HS, K, split, hbj)
    T = RS.rescale_target(f["rew"].double(), f["gam"].double(), r0["q_g"][torch.arange(B), r0["astar"]], EPS32)
    r = F.head_oracle(hbj[:2 * B], hbj[2 * B:], f["Pon"], f["Ptg"], f["act"], T, torch.zeros(B), f["isw"], True, F.KAPPA,
                      1.0 / B)
    assert r0["gap"] > F.MARGIN / 2 and r["kmargin"] > F.MARGIN / 2
    D._compare(oa, r, split, f"rescaled fc + head, deferred (split {split})")
    assert float((r["td"] - r0["td"]).abs().max()) > 0.1


# ------------------------------------------------------------------ 3. quantile head
_QR_CASE_INPUTS = QR._case_inputs


def _qr_case_inputs(fx, case):
    """The cases of tests/test_gpu_qr.py and ``saturated``: R = +-1e4 by turns, targets of about +-109."""
    if case != "saturated":
        return _QR_CASE_INPUTS(fx, case)
    rew = torch.full((fx["act"].shape[0],), 1e4)
    rew[1::2] = -1e4
    return rew, fx["gam"], fx["isw"]


def _qr(B, A, N, split, case):
    r = QR._oracle.__wrapped__(B, A, N, split, case)
    h = QR._run_hip(B, A, N, split, case)
    return h, r


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", [(5, 3, 2), (33, 4, 32), (7, 18, 64)])
@pytest.mark.parametrize("case", ["plain", "terminal", "saturated"])
def test_quantile_head_vs_fp64_oracle(rescaled, monkeypatch, B, A, N, case, split):
    """Odd B: the second sample slot of the last block is empty.  ``terminal``: every T_j = h(R); ``saturated``
    (R = +-1e4): every |u| is past kappa.  td_abs against the mean of the transformed T_j."""
    monkeypatch.setattr(QR, "_case_inputs", _qr_case_inputs)
    h, r = _qr(B, A, N, split, case)
    assert r["gap"] > 1e-3
    QR._compare(h, r)
    assert h["zeroed"]
    fx = QR._fixture(B, A, N, split)
    rew, gam, _ = QR._case_inputs(fx, case)
    T = RS.rescale_target(rew.double()[:, None], gam.double()[:, None], r["th_target"], EPS)
    td = (T.mean(-1) - r["th"].mean(-1)).abs()
    torch.testing.assert_close(r["td"], td, rtol=1e-12, atol=1e-12)
    if case == "plain" and N >= 32:      # the shortcut through the mean of the target's quantiles is another number
        short = (RS.rescale_target(rew.double(), gam.double(), r["th_target"].mean(-1), EPS) - r["th"].mean(-1)).abs()
        assert float((short - td).abs().max()) > 1e-3
    if case == "saturated":
        assert float((T[:, :, None] - r["th"][:, None, :]).abs().min()) > 50 * QR.KAPPA
        assert 100 < float(T.abs().min()) and float(T.abs().max()) < 120


# ------------------------------------------------------------------ 4. implicit quantile head
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N,max_blocks", [(5, 3, 5, None), (33, 4, 8, None), (13, 4, 8, 3)])
def test_implicit_head_and_wgrad_vs_fp64_oracle(rescaled, B, A, N, max_blocks, split):
    r = FI.run_torch(B, A, N, split)
    h = IQ._run_hip(B, A, N, split, max_blocks=max_blocks)
    assert r["gap"] > 1e-3
    assert torch.equal(h["taus"], r["taus"])                  # still bit-equal to the mirror
    assert h["zeroed"]
    FI.compare(h, r)
    fx = FI.fixture(B, A, split)
    T = RS.rescale_target(fx["rew"].double()[:, None], fx["gam"].double()[:, None], r["th_target"], EPS)
    torch.testing.assert_close(r["td"], (T.mean(-1) - r["th"].mean(-1)).abs(), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ 5. categorical head
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", [(33, 4, 51), (5, 6, 7)])
def test_categorical_head_vs_fp64_oracle(rescaled, B, A, N, split):
    """Rows 1 and 2 carry R = +-400: every transformed atom of them clamps at v_max / v_min; the other rows'
    atoms lie inside the support."""
    fx = C51._fixture(B, A, N, split)
    rew = fx["rew"].clone()
    rew[1], rew[2] = 400.0, -400.0
    z = C51.VMIN + torch.arange(N, dtype=torch.float64) * ((C51.VMAX - C51.VMIN) / (N - 1))
    tz = RS.rescale_target(rew.double()[:, None], fx["gam"].double()[:, None], z[None, :], EPS)
    assert bool((tz[1] > C51.VMAX).all()) and bool((tz[2] < C51.VMIN).all())
    assert bool(((tz[3:] > C51.VMIN) & (tz[3:] < C51.VMAX)).any())
    r = C51._oracle(fx, A, N, rew=rew)
    h = C51._run_hip(fx, A, N, rew=rew)
    assert r["gap"] > 1e-3
    C51._compare(h, r)
    assert h["zeroed"]


# ------------------------------------------------------------------ 6. whole step
def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"value_rescale": True, **rt}})


def _fill_replay(rp, K, A=6, seed=0):
    """tests/head_fixtures.py ``fill_replay`` with raw rewards of either sign up to about 100."""
    rng = np.random.default_rng(seed)
    seqs = rp.append_frames(rng.integers(0, 255, (K + 8, 84, 84), dtype=np.uint8))
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, A, K), R=(rng.normal(size=K) * 30).astype(np.float32),
                   Gamma=np.where(rng.random(K) < 0.1, 0.0, 0.97).astype(np.float32),
                   priority=rng.random(K).astype(np.float32) * 3 + 0.01))


@pytest.mark.parametrize("dtype,rt", [("bf16", {}), ("fp32", {}), ("fp32", {"num_atoms": 32, "dist_head": "quantile"}),
                                      ("bf16", {"noisy": True})])
def test_learner_step_hip_vs_torch_backend(dtype, rt):
    """tests/test_gpu_qr.py test_qr_learner_step_hip_vs_torch_backend with the key on, at that test's shapes
    and bounds."""
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, **rt)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        _fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.rescale_eps == EPS and L.split == split
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, float(L.gnorm), gn)
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout, L.S["rew"].clone())
    assert torch.equal(res["hip"][2], res["torch"][2])
    assert float(res["hip"][5].abs().max()) > 30 and float(res["hip"][0].max()) < 30     # |R| up to ~100, td squashed
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} {rt} HIP step vs the torch backend):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0


def test_graph_of_four_updates_is_bit_identical_to_four_eager_steps():
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res = {}
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        _fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        if graphs:
            L.steps(4)
            assert L._multi is not None
        else:
            for _ in range(4):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 4
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.S["idx"].clone(), L.td_abs.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_gpu_resume_is_bit_identical(tmp_path):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

    def replay():
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=5)
        _fill_replay(rp, 1500, seed=2)
        return rp
    cfg = _cfg(32, use_graphs=True, graph_steps=4, learner={"q_target_sync_freq": 3})
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
    assert d["Runtime"]["value_rescale"] is True
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.num_q_updates == 3 and L2.rescale_eps == EPS
    for _ in range(3):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.td_abs, L2.td_abs)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. GPU loop
def test_gpu_loop_on_unclipped_fake_ale_inserts_the_numpy_builders_priorities(monkeypatch):
    """Lock-step on ``fake_ale`` with ``clip_rewards`` false: the actor group's builder (the native one where
    the host runtime is built) is shadowed by the numpy builder fed the same steps; every batch the group
    inserts carries the numpy builder's priorities, and raw rewards of 5 reach the replay."""
    from apex_dqn_amd.actors import gpu_actor
    from apex_dqn_amd.actors.nstep import NStepBuilder
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    real = gpu_actor.make_nstep_builder
    seen = dict(batches=0, rows=0, eps=set(), rmax=0.0)

    class Tee:
        def __init__(self, *a, **kw):
            self.a = real(*a, **kw)
            kw2 = dict(kw)
            self.b = NStepBuilder(*a, **kw2)
            self.env_ids = self.a.env_ids
            seen["eps"].add(kw.get("value_rescale_eps"))

        def step(self, *a):
            self.a.step(*a)
            self.b.step(*a)

        @property
        def size(self):
            return self.a.size

        def get(self, max_items=None):
            x, y = self.a.get(max_items), self.b.get(max_items)
            assert (x is None) == (y is None)
            if x is not None:
                for k in x:
                    assert np.array_equal(x[k], y[k]), k
                seen["batches"] += 1
                seen["rows"] += len(x["A_t"])
                seen["rmax"] = max(seen["rmax"], float(np.abs(x["R"]).max()))
                # on the rescaled scale: a plain n-step priority of these returns would reach |R| itself
                assert np.isfinite(x["priority"]).all()
            return x
    monkeypatch.setattr(gpu_actor, "make_nstep_builder", Tee)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "PongNoFrameskip-v4"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16, "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 8, "q_target_sync_freq": 5},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 20, "use_graphs": True, "env_backend": "fake_ale",
                                            "value_rescale": True, "clip_rewards": False}})
    out = train_frames(cfg, DEV, 20, num_envs=16, async_actors=False)
    L, rp = out["learner"], out["replay"]
    torch.cuda.synchronize()
    assert L.rescale_eps == EPS and L.num_q_updates == 20
    assert seen["eps"] == {EPS} and seen["batches"] > 10 and seen["rows"] >= 300
    assert seen["rmax"] > 1.0
    assert float(rp.rew.abs().max()) > 1.0                                # stored raw
    live = rp.leaf[rp.leaf != 0]
    assert live.numel() >= 300 and bool(torch.isfinite(live).all()) and bool((live > 0).all())
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
