"""Munchausen-IQN (``Runtime.dist_head = "implicit_munchausen"``, csrc/iqn_wide_head.hip miqn_wide_finish_kernel) without
a GPU: the target by hand, the torch backend against autograd, the kind's validation, checkpoints and one MLP step, and
the problems, fp64 oracle, fixture conditions and measured allowances that tests/test_gpu_miqn.py uses."""
import functools
import math
import os

import iqn_fixtures as F
import pytest
import torch
from test_iqn_cpu import _problem, _theta
from test_iqn_wide_cpu import _hilo

from apex_dqn_amd.learner import iqn
from apex_dqn_amd.learner.losses import miqn_loss, miqn_targets, tau_log_policy

MK = dict(alpha=0.9, tau=0.03, clip=-1.0)
# (B, A, N): a ragged finish block below one 16-sample tile; one action (pi = 1, bonus = 0) with a clamped tail tile;
# stride 64 with one full register set; stride 256, NQ = 2; two 16-row head tiles, NQ = 4
SHAPES = [(5, 3, 2), (4, 1, 17), (6, 4, 64), (3, 4, 65), (2, 18, 256)]
ADV_SCALE = {(6, 4): 0.02, (3, 4): 0.02}           # (B, A): target advantage head scaled: action gaps of the order of tau_m
CASES = {"alpha0": dict(alpha=0.0), "tau1": dict(tau=1.0)}      # beside iqn_fixtures' "terminal" and "no_isw"
EDGE = (6, 4, 64)
OUTS = ("td", "loss", "dhead", "bonus", "vsoft")


@functools.lru_cache(maxsize=None)
def fixture(B, A, split=False):
    """``iqn_fixtures.fixture`` on the Munchausen row plan: Hon [B] = its online S_t rows, Htg [2B] = its target rows
    (S_t+n), then its online S_t+n rows standing in for the target net's S_t input."""
    fx, s = F.fixture(B, A, split), ADV_SCALE.get((B, A), 1.0)
    cat = lambda a, b: None if a is None else torch.cat([a, b[B:]])      # noqa: E731
    Ptg = {**fx["Ptg"], "wa": fx["Ptg"]["wa"] * s, "ba": fx["Ptg"]["ba"] * s}
    return {**fx, "Ptg": Ptg, "Hon": fx["Hon"][:B], "Hon_lo": None if fx["Hon_lo"] is None else fx["Hon_lo"][:B],
            "Htg": cat(fx["Htg"], fx["Hon"]), "Htg_lo": cat(fx["Htg_lo"], fx["Hon_lo"])}



@functools.lru_cache(maxsize=None)
def oracle(B, A, N, split=False, case="plain", emulate=False):
    """The fp64 torch backend on ``fixture`` (computed once, shared, never modified).  ``emulate``: We, the cosines, wv
    and wa rounded to bf16 hi + lo as the kernels' products take them (tests/test_iqn_wide_cpu.py), the rest fp64."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be, fx, mk = TorchBackend(torch.float64), fixture(B, A, split), {**MK, **CASES.get(case, {})}
    rew, gam, isw = F.case_inputs(fx, "plain" if case in CASES else case)
    d = lambda t: t.double()                                             # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi) + d(lo)        # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    rnd = (lambda k, v: _hilo(v) if k in ("wv", "wa", "wtau") else d(v)) if emulate else (lambda k, v: d(v))
    Pon, Ptg, Eon, Etg = ({k: rnd(k, v) for k, v in fx[n].items()} for n in ("Pon", "Ptg", "Eon", "Etg"))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                  # noqa: E731
    td, loss, dH, dhead, q, aux = z(B), z(B), z(B, 1024), z(B, (A + 1) * N), z(B, A), z(B, 2)
    taus, ws = torch.zeros(B, 3, N), be.iqn_workspace(B, N, "cpu", torch.float64)
    cos = iqn.cos_features
    if emulate:
        iqn.cos_features = lambda tau, dtype=torch.float64: _hilo(cos(tau, torch.float64)).to(dtype)
    try:
        be.miqn_head(Hon, Htg, Pon, Ptg, Eon, Etg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, F.KAPPA,
                     mk["alpha"], mk["tau"], mk["clip"], 1.0 / B, F.seed_q(), torch.tensor([F.CTR]),
                     torch.tensor([F.BASE]), td, loss, dH, dhead, ws, aux=aux, q_out=q, tau_out=taus)
        pre = be._iqn_theta(Hon, Pon, Eon, taus[:, 0], torch.float64)[1]
        g0 = be._iqn_theta(Htg[B:], Ptg, Etg, taus[:, 1], torch.float64)[0].mean(-1)
        g1 = be._iqn_theta(Htg[:B], Ptg, Etg, taus[:, 2], torch.float64)[0].mean(-1)
    finally:
        iqn.cos_features = cos
    gr = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
    be.iqn_wgrad(fx["act"], ws, gr)
    g = dhead[:, :N]
    coef = torch.nn.functional.one_hot(fx["act"].long(), A).double() - 1.0 / A
    dx = torch.cat([g[:, :, None] * Pon["wv"].reshape(512), g[:, :, None] * (coef @ Pon["wa"])[:, None, :]], -1)
    tl0 = tau_log_policy(g0, mk["tau"]).gather(1, fx["act"].long()[:, None]).squeeze(1)
    return dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, taus=taus, bonus=aux[:, 0], vsoft=aux[:, 1], pre=pre,
                unmasked=(dx * Hon[:, None, :]).abs(), clip_margin=float((tl0 - mk["clip"]).abs().min()),
                maxpi=(tau_log_policy(g1, mk["tau"]) / mk["tau"]).exp().max(1).values)


def allowances(B, A, N, split=False, case="plain"):
    """Per output of ``OUTS``: 4 x the largest deviation of the emulated split-bf16 operands from the exact ones (the
    softmax amplifies their rounding by 1 / tau_m), and the kink band of tests/test_iqn_wide_cpu.py ``allowances``."""
    r, e = oracle(B, A, N, split, case), oracle(B, A, N, split, case, emulate=True)
    return ({k: 4 * float((e[k] - r[k]).abs().max()) for k in OUTS},
            max(F.KINK, 4 * float((e["pre"] - r["pre"]).abs().max())))


def compare(h, r, al, band):
    """``iqn_fixtures.compare``'s bounds (the wide implicit head's), the absolute ones of td, loss, dhead raised by
    ``al``; bonus and vsoft take q's bound plus theirs; the wtau / btau slack is the unmasked gradient inside ``band``."""
    f = lambda t: t.float()                                              # noqa: E731
    print("kernel error per output:", {k: f"{float((h[k].double() - r[k]).abs().max()):.2e}" for k in OUTS}, "allowed:", al)
    torch.testing.assert_close(f(h["td"]), f(r["td"]), rtol=1e-4, atol=1e-4 + al["td"])
    torch.testing.assert_close(f(h["loss"]), f(r["loss"]), rtol=1e-4, atol=1e-5 + al["loss"])
    torch.testing.assert_close(f(h["dhead"]), f(r["dhead"]), rtol=1e-4, atol=1e-7 + al["dhead"])
    for k in ("bonus", "vsoft"):
        torch.testing.assert_close(f(h[k]), f(r[k]), rtol=1e-4, atol=1e-4 + al[k])
    F.compare({**h, **{k: f(r[k]) for k in ("td", "loss", "dhead")}},
              {**r, "slack": (r["unmasked"] * (r["pre"].abs() < band)).sum((0, 1))})


def test_miqn_targets_by_hand():
    """A clipped row, an unclipped row and a terminal row, written out with ``math``; mean_j T_j = R + bonus + Gamma vsoft."""
    tau, alpha, clip = 0.5, 0.9, -1.0
    th0 = torch.tensor([[[0.0, 2.0], [3.0, 5.0]], [[1.0, 1.2], [1.1, 1.3]], [[0.3, 0.1], [0.2, 0.6]]], dtype=torch.float64)
    th1 = torch.tensor([[[1.0, 3.0], [0.5, 1.5]], [[2.0, 0.0], [1.5, 2.5]], [[9.0, 9.0], [1.0, 1.0]]], dtype=torch.float64)
    A, R, G = torch.tensor([0, 1, 0]), torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64), torch.tensor(
        [0.9, 0.97, 0.0], dtype=torch.float64)
    T, bonus, vsoft = miqn_targets(th0, th1, A, R, G, alpha, tau, clip)

    def tlp(g):
        m = max(g)
        ls = math.log(sum(math.exp((x - m) / tau) for x in g))
        return [(x - m) - tau * ls for x in g]
    for b in range(3):
        g0, g1 = [float(th0[b, a].mean()) for a in range(2)], [float(th1[b, a].mean()) for a in range(2)]
        t0, t1 = tlp(g0)[int(A[b])], tlp(g1)
        want_bonus = alpha * min(max(t0, clip), 0.0)
        assert (t0 < clip) == (b == 0)
        pi = [math.exp(t / tau) for t in t1]
        for j in range(2):
            mix = sum(pi[a] * (float(th1[b, a, j]) - t1[a]) for a in range(2))
            assert abs(float(T[b, j]) - (float(R[b]) + want_bonus + float(G[b]) * mix)) < 1e-12
        assert abs(float(bonus[b]) - want_bonus) < 1e-12
        assert abs(float(vsoft[b]) - sum(pi[a] * (g1[a] - t1[a]) for a in range(2))) < 1e-12
    torch.testing.assert_close(T.mean(-1), R + bonus + G * vsoft, rtol=1e-12, atol=1e-12)
    assert float(T[2].sub(R[2] + bonus[2]).abs().max()) == 0.0           # terminal: no next-state term


@pytest.mark.parametrize("A,N", [(4, 8), (3, 5)])
def test_torch_backend_backward_matches_autograd(A, N):
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    B, seed, u = 6, iqn.iqn_seed(5), 4
    pr, be = _problem(B, A, N, 10 + A), TorchBackend(torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                  # noqa: E731
    td, loss, dH, dhead, q, aux = z(B), z(B), z(B, 1024), z(B, (A + 1) * N), z(B, A), z(B, 2)
    taus, ws = torch.zeros(B, 3, N), be.iqn_workspace(B, N, "cpu", torch.float64)
    h_tg = torch.relu(torch.cat([pr["z_tg"], pr["z_on"][B:]]))           # target rows: S_t+n, then S_t
    be.miqn_head(torch.relu(pr["z_on"][:B]), h_tg, pr["Pon"], pr["Ptg"], pr["Eon"], pr["Etg"], pr["act"], pr["rew"],
                 pr["gam"], pr["isw"], N, 1.0, 0.9, 0.5, -1.0, 1.0 / B, seed, torch.tensor([u + 2]), torch.tensor([2]), td,
                 loss, dH, dhead, ws, aux=aux, q_out=q, tau_out=taus)
    gr = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
    be.iqn_wgrad(pr["act"], ws, gr)
    assert torch.equal(taus, iqn.learner_taus(seed, u, B, N))
    zt = pr["z_on"][:B].clone().requires_grad_(True)
    P = {k: v.clone().requires_grad_(True) for k, v in pr["Pon"].items()}
    E = {k: v.clone().requires_grad_(True) for k, v in pr["Eon"].items()}
    th_t = _theta(torch.relu(zt), P, E, taus[:, 0])
    with torch.no_grad():
        th1 = _theta(h_tg[:B], pr["Ptg"], pr["Etg"], taus[:, 2])
        th0 = _theta(h_tg[B:], pr["Ptg"], pr["Etg"], taus[:, 1])
    L, td_ref = miqn_loss(th_t, taus[:, 0], th0, th1, pr["act"], pr["rew"], pr["gam"], 1.0, pr["isw"], 0.9, 0.5, -1.0)
    L.backward()
    tol = dict(rtol=1e-10, atol=1e-13)
    ref = miqn_targets(th0, th1, pr["act"], pr["rew"], pr["gam"], 0.9, 0.5, -1.0)
    for got, want in ((td, td_ref), (loss.mean(), L.detach()), (q, th_t.detach().mean(-1)), (dH, zt.grad),
                      (aux[:, 0], ref[1]), (aux[:, 1], ref[2]), *((gr[k], P[k].grad) for k in P),
                      *((gr[k], E[k].grad) for k in E)):
        torch.testing.assert_close(got, want, **tol)
    assert float(E["wtau"].grad.abs().max()) > 0 and float(zt.grad.abs().max()) > 0


def _cfg(**rt):
    from apex_dqn_amd.config import ApexConfig
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4], "action_dim": 2, "name": "CartPole-v1"},
                                 "Runtime": {"num_atoms": 8, "dist_head": "implicit_munchausen", "iqn_wide": True, **rt}})


def test_kind_refusals_shipped_config_checkpoints_and_one_mlp_step(tmp_path):
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.torch_learner import TorchLearner
    cfg = _cfg()
    assert cfg.miqn and cfg.implicit and cfg.wide_implicit and cfg.head_kw()["dist_head"] == "implicit"
    assert not _cfg(dist_head="implicit").miqn
    for key, bad in (("iqn_wide", dict(iqn_wide=False)), ("munchausen", dict(munchausen=True)), ("noisy", dict(noisy=True)),
                     ("value_rescale", dict(value_rescale=True)), ("munchausen_tau", dict(munchausen_tau=0.0)),
                     ("munchausen_alpha", dict(munchausen_alpha=1.5)), ("munchausen_clip", dict(munchausen_clip=0.0))):
        with pytest.raises(ValueError, match="Runtime." + key):
            _cfg(**bad)
    rt = ApexConfig.load(os.path.join(os.path.dirname(__file__), "..", "configs", "pong_1gpu_miqn.json")).Runtime
    assert (rt.num_atoms, rt.dist_head, rt.iqn_wide, rt.optimizer) == (64, "implicit_munchausen", True, "adam")
    assert (rt.munchausen_alpha, rt.munchausen_tau, rt.munchausen_clip) == (0.9, 0.03, -1.0)
    T, g, B = TorchLearner(cfg, "cpu"), torch.Generator().manual_seed(3), 16
    out = T.step(dict(S_t=torch.randn(B, 4, generator=g), S_tpn=torch.randn(B, 4, generator=g),
                      A_t=torch.randint(0, 2, (B,), generator=g), R=torch.rand(B, generator=g), Gamma=torch.full((B,), 0.97),
                      weights=torch.ones(B)))
    assert math.isfinite(out["loss"]) and out["munchausen_bonus_mean"] <= 0.0 and math.isfinite(out["soft_value_mean"])
    # the kinds share keys and shapes but not the target: refused in both directions
    plain = TorchLearner(_cfg(dist_head="implicit"), "cpu")
    for src, dst, name in ((T, plain, "m.pt"), (plain, T, "p.pt")):
        src.save(str(tmp_path / name))
        with pytest.raises(ValueError, match="dist_head"):
            dst.load(str(tmp_path / name))


@pytest.mark.parametrize("B,A,N", SHAPES)
def test_fixture_conditions_and_allowances_of_the_gpu_shapes(B, A, N):
    """By the oracle alone, no row excluded: tau ln pi0[a_b] stays 2e-3 off the clip, at most 10 % of the embedding rows
    carry near-kink slack, the scaled fixtures' mixture is not one-hot, and the measured allowances, printed."""
    for split in (False, True):
        r = oracle(B, A, N, split)
        al, band = allowances(B, A, N, split)
        share = float((r["pre"].abs() < F.KINK).any(0).any(0).float().mean())
        print(f"{(B, A, N)} split {split}: clip margin {r['clip_margin']:.2e}, kink share {share:.3f}, band {band:.2e}, "
              f"soft rows {int((r['maxpi'] < 0.9).sum())}/{B}, allowances {al}")
        assert r["clip_margin"] > 2e-3 and share <= 0.10
        assert all(math.isfinite(v) for v in al.values())
        if (B, A) in ADV_SCALE:
            assert int((r["maxpi"] < 0.9).sum()) * 4 >= B
    for case in ("terminal", "no_isw", *CASES):
        assert oracle(*EDGE, False, case)["clip_margin"] > 2e-3
