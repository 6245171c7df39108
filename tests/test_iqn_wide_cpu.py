"""``Runtime.iqn_wide`` (the implicit quantile head with up to 256 samples, csrc/iqn_wide_head.hip) without a GPU: the
key's validation, the tau draws' stride, the shipped config, one MLP torch step at N = 72, and the problems, the fp64
oracle and the CPU emulation of the kernels' product rule that tests/test_gpu_iqn_wide.py uses."""
import functools
import os

import iqn_fixtures as F
import numpy as np
import pytest
import torch

from apex_dqn_amd.learner import iqn

# (B, A, N): N below one 16-sample MFMA tile; A > 16 (two action tiles) and a full register set; one sample in the
# second register set, ragged tiles, stride 256; the paper-sized middle; A = 1 (the dueling mean is the identity) at
# the largest N
SHAPES = [(5, 4, 8), (13, 18, 64), (3, 2, 65), (7, 6, 200), (4, 1, 256)]
EDGE = (7, 6, 200)
EPS = 1e-2      # the rescaled edge case's Runtime.value_rescale


def _hilo(v):
    """v as the MFMAs see it: bf16 hi + bf16 lo of the fp32 value (2^-17 relative), in fp64."""
    v = v.float()
    hi = v.bfloat16().float()
    return hi.double() + (v - hi).bfloat16().double()


@functools.lru_cache(maxsize=None)
def oracle(B, A, N, split=False, case="plain", kappa=F.KAPPA, eps=None, emulate=False):
    """``iqn_fixtures.run_torch`` in fp64 on ``iqn_fixtures.fixture`` (computed once, shared, never modified), with
    A = 1 (no top-2 gap there), ``rescale_eps``, and ``pre`` / ``unmasked`` of set 0 kept for the kink band.
    ``emulate``: We, the cosines, wv and wa rounded to bf16 hi + lo as the kernels' products take them, the rest fp64."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be, fx = TorchBackend(torch.float64), F.fixture(B, A, split)
    rew, gam, isw = F.case_inputs(fx, case)
    d = lambda t: t.double()                                             # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi) + d(lo)        # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    rnd = (lambda k, v: _hilo(v) if k in ("wv", "wa", "wtau") else d(v)) if emulate else (lambda k, v: d(v))
    Pon, Ptg, Eon, Etg = ({k: rnd(k, v) for k, v in fx[n].items()} for n in ("Pon", "Ptg", "Eon", "Etg"))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                  # noqa: E731
    td, loss, dH, dhead, q = z(B), z(B), z(B, 1024), z(B, (A + 1) * N), z(B, A)
    taus, ws = torch.zeros(B, 3, N), be.iqn_workspace(B, N, "cpu", torch.float64)
    cos = iqn.cos_features
    if emulate:
        iqn.cos_features = lambda tau, dtype=torch.float64: _hilo(cos(tau, torch.float64)).to(dtype)
    try:
        be.iqn_head(Hon, Htg, Pon, Ptg, Eon, Etg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, kappa,
                    1.0 / B, F.seed_q(), torch.tensor([F.CTR]), torch.tensor([F.BASE]), td, loss, dH, dhead, ws, q_out=q,
                    tau_out=taus, rescale_eps=eps)
        qn = be._iqn_theta(Hon[B:2 * B], Pon, Eon, taus[:, 1], torch.float64)[0].mean(-1)
        pre = be._iqn_theta(Hon[:B], Pon, Eon, taus[:, 0], torch.float64)[1]
    finally:
        iqn.cos_features = cos
    gr = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
    be.iqn_wgrad(fx["act"], ws, gr)
    top = qn.topk(min(A, 2), dim=1).values
    g = dhead[:, :N]
    coef = torch.nn.functional.one_hot(fx["act"].long(), A).double() - 1.0 / A
    dx = torch.cat([g[:, :, None] * Pon["wv"].reshape(512), g[:, :, None] * (coef @ Pon["wa"])[:, None, :]], -1)
    return dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, taus=taus, pre=pre,
                unmasked=(dx * Hon[:B, None, :]).abs(), gap=float((top[:, 0] - top[:, -1]).min()) if A > 1 else float("inf"))


def allowances(r, e):
    """(dhead floor, kink band) of a problem from its oracle ``r`` and emulation ``e``: 4 x the emulated product
    rule's dhead error, and 4 x its largest |pre_emulated - pre_fp64| where that exceeds the fixture's ``KINK``."""
    return 4 * float((e["dhead"] - r["dhead"]).abs().max()), max(F.KINK, 4 * float((e["pre"] - r["pre"]).abs().max()))


def compare(h, r, e):
    """``iqn_fixtures.compare`` with the two allowances, both taken from the references: dhead's absolute bound is
    the floor where that is above 1e-7, and the wtau / btau slack is the unmasked gradient inside the kink band."""
    floor, band = allowances(r, e)
    slack = (r["unmasked"] * (r["pre"].abs() < band)).sum((0, 1))
    print(f"emulated product rule: dhead floor {floor:.2e}, kink band {band:.2e}; kernel dhead err "
          f"{float((h['dhead'].double() - r['dhead']).abs().max()):.2e}; errors / iqn_fixtures tolerance (dhead without the "
          f"floor) { {k: round(v, 3) for k, v in F.max_errors(h, {**r, 'slack': slack}).items()} }")
    torch.testing.assert_close(h["dhead"].float(), r["dhead"].float(), rtol=1e-4, atol=max(1e-7, floor))
    F.compare({**h, "dhead": r["dhead"].float()}, {**r, "slack": slack})


def _cfg(**rt):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 4, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": 8}, "Runtime": rt})


def test_key_validation_and_round_trip():
    from apex_dqn_amd.config import ApexConfig
    for n in (2, 64, 65, 256):
        cfg = _cfg(num_atoms=n, dist_head="implicit", iqn_wide=True)
        assert cfg.wide_implicit and ApexConfig.from_dict(cfg.to_dict()).Runtime.iqn_wide is True
    assert not _cfg(num_atoms=8, dist_head="implicit").wide_implicit
    for bad in (dict(num_atoms=1), dict(num_atoms=32, dist_head="quantile"), dict(num_atoms=32, dist_head="categorical"),
                dict(num_atoms=32, dist_head="hl_gauss"), dict(num_atoms=8, dist_head="implicit", iqn_wide=1)):
        with pytest.raises(ValueError, match="iqn_wide"):
            _cfg(**{"iqn_wide": True, **bad})
    with pytest.raises(ValueError, match="num_atoms"):
        _cfg(num_atoms=257, dist_head="implicit", iqn_wide=True)
    # off: the two pinned refusals hold, and 65 names the key
    with pytest.raises(ValueError, match="num_atoms.*iqn_wide"):
        _cfg(num_atoms=65, dist_head="implicit")
    with pytest.raises(ValueError, match="wide_atoms"):
        _cfg(num_atoms=32, dist_head="implicit", wide_atoms=True)
    with pytest.raises(ValueError, match="iqn_actor_samples"):      # the actors keep their range
        _cfg(num_atoms=128, dist_head="implicit", iqn_wide=True, iqn_actor_samples=65)
    for k in ("noisy", "munchausen"):
        with pytest.raises(ValueError, match="Runtime." + k):
            _cfg(num_atoms=128, dist_head="implicit", iqn_wide=True, **{k: True})


@pytest.mark.parametrize("N", [2, 8, 64, 65, 256])
def test_learner_taus_stride(N):
    """Stride 64 up to N = 64 (the values of before: the narrow kernel's fractions), 256 above; the 3 B N indices are
    distinct, so no two sets share a draw."""
    from apex_dqn_amd.replay.gpu_replay import apex_uniform
    B, u, seed = 5, 7, F.seed_q()
    stride = 64 if N <= 64 else 256
    assert iqn.learner_stride(N) == stride
    idx = np.arange(3 * B, dtype=np.uint64)[:, None] * np.uint64(stride) + np.arange(N, dtype=np.uint64)[None, :]
    assert np.unique(idx).size == 3 * B * N
    want = torch.from_numpy(apex_uniform(seed, 64 * u, idx).reshape(B, 3, N).copy())
    assert torch.equal(iqn.learner_taus(seed, u, B, N), want)


def test_shipped_config_and_one_mlp_torch_step_at_72_samples():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.torch_learner import TorchLearner
    rt = ApexConfig.load(os.path.join(os.path.dirname(__file__), "..", "configs", "pong_1gpu_iqn_wide.json")).Runtime
    assert (rt.num_atoms, rt.dist_head, rt.iqn_wide, rt.optimizer) == (64, "implicit", True, "adam")
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                "Runtime": {"num_atoms": 72, "dist_head": "implicit", "iqn_wide": True}})
    assert cfg.network == "mlp"
    T, g, B = TorchLearner(cfg, "cpu"), torch.Generator().manual_seed(3), 16
    out = T.step(dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                      A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g), Gamma=torch.full((B,), 0.97),
                      weights=torch.ones(B)))
    assert T.last_taus.shape == (B, 3, 72) and np.isfinite(out["loss"]) and np.isfinite(out["td_abs"]).all()
    assert torch.equal(T.last_taus, iqn.learner_taus(iqn.iqn_seed(cfg.Runtime.seed), 0, B, 72))


@pytest.mark.parametrize("B,A,N", SHAPES)
def test_fixture_conditions_of_the_gpu_shapes(B, A, N):
    """No near-tie in a* on any compared problem (the top-2 gap of the online next-state q is above the q tolerance),
    the emulated product rule picks the oracle's a*, and the two allowances it yields, printed."""
    for split in (False, True):
        r, e = oracle(B, A, N, split), oracle(B, A, N, split, emulate=True)
        floor, band = allowances(r, e)
        print(f"{(B, A, N)} split {split}: gap {r['gap']:.2e}, dhead floor {floor:.2e}, kink band {band:.2e}")
        assert r["gap"] > 1e-3 and e["gap"] > 1e-3          # ten times the q tolerance
        if A > 1:
            assert torch.equal(r["taus"], F.oracle(B, A, N, split)["taus"])
            assert torch.equal(r["dhead"], F.oracle(B, A, N, split)["dhead"])       # the frame is iqn_fixtures'
