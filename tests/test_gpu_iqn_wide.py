"""Wide implicit quantile head (``Runtime.iqn_wide``, csrc/iqn_wide_head.hip) on the GPU: the three launches and the
weight gradient against the fp64 oracle on tests/iqn_fixtures.py's problems, the narrow kernel on a shared shape, the
launcher's refusals, the whole step against the torch backend and graph replay against eager steps.
tests/test_iqn_wide_cpu.py holds the shapes, the oracle, the CPU emulation of the product rule and the two allowances
derived from it."""
import functools

import iqn_fixtures as F
import pytest
import torch
from test_gpu_iqn import DEV, _cfg, _fill_replay, _run_hip
from test_iqn_wide_cpu import EDGE, EPS, SHAPES, compare, oracle

pytestmark = pytest.mark.gpu


@pytest.fixture
def wide(monkeypatch):
    """tests/test_gpu_iqn.py's ``_run_hip`` through the wide launches."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    narrow = HipBackend.iqn_head

    def on(**kw):
        monkeypatch.setattr(HipBackend, "iqn_head", functools.partialmethod(narrow, wide=True, **kw))
    on()
    return on


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", SHAPES)
def test_iqn_wide_head_and_wgrad_vs_fp64_oracle(B, A, N, split, wide):
    """``iqn_fixtures.compare``'s bounds with the two allowances of tests/test_iqn_wide_cpu.py ``compare``.  Measured
    there (fp64, CPU; bf16 / split agree to two digits): 4 x the emulated product rule's dhead error is 1.2e-6, 1.0e-6,
    0, 9.1e-7 and 1.0e-6 in the order of ``SHAPES``, and the kink band (4 x its largest |pre_emulated - pre_fp64|)
    5.1e-5, 4.9e-5, 4.3e-5, 4.9e-5 and 5.3e-5."""
    r, h = oracle(B, A, N, split), _run_hip(B, A, N, split)
    assert torch.equal(h["taus"], r["taus"]) and h["zeroed"]
    compare(h, r, oracle(B, A, N, split, emulate=True))


def test_iqn_wide_draws_the_narrow_kernels_fractions(monkeypatch):
    """At N <= 64 the key compares the two paths on one shape: the same fractions bit for bit, td / loss / q within
    ``iqn_fixtures.compare``'s bounds of each other."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    B, A, N = SHAPES[0]
    narrow = _run_hip(B, A, N)
    monkeypatch.setattr(HipBackend, "iqn_head", functools.partialmethod(HipBackend.iqn_head, wide=True))
    h = _run_hip(B, A, N)
    assert torch.equal(h["taus"], narrow["taus"])
    torch.testing.assert_close(h["td"], narrow["td"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(h["loss"], narrow["loss"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(h["q"], narrow["q"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("case", ["terminal", "no_isw", "kappa", "rescale_eps"])
def test_iqn_wide_edge_cases(case, wide):
    """All-terminal rows, weights off, kappa = 0.25, and the RESCALE instantiation with split inputs and the IS
    statistic (equal to the oracle's exactly)."""
    B, A, N = EDGE
    if case == "rescale_eps":
        wide(rescale_eps=EPS)
        h = _run_hip(B, A, N, True, isn=True)
        compare(h, oracle(B, A, N, True, eps=EPS), oracle(B, A, N, True, eps=EPS, emulate=True))
        assert h["count"] == B and h["isn"] == float(F.fixture(B, A, True)["isw"].max().double() / F.WSCALE)
        return
    kappa = 0.25 if case == "kappa" else F.KAPPA
    r, h = oracle(B, A, N, False, case, kappa), _run_hip(B, A, N, False, case, kappa)
    compare(h, r, oracle(B, A, N, False, case, kappa, emulate=True))
    if case == "terminal":
        qa = r["q"][torch.arange(B), F.fixture(B, A)["act"].long()]
        torch.testing.assert_close(h["td"], (F.fixture(B, A)["rew"].double() - qa).abs().float(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("bad", ["N", "null"])
def test_iqn_wide_launcher_refuses(bad):
    """N = 257 and a null output each return hipErrorInvalidValue (1) and launch nothing: the outputs keep their fill."""
    from apex_dqn_amd.ops import _lib
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be, (B, A, N) = HipBackend(), (4, 2, 65)
    fx = F.fixture(B, A)
    d = lambda v: v.to(DEV)                                              # noqa: E731
    Pon, Ptg = {k: d(v) for k, v in fx["Pon"].items()}, {k: d(v) for k, v in fx["Ptg"].items()}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH, dhead = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16), torch.full((B, (A + 1) * N), 7.0, device=DEV)
    keep = [d(fx[k]) for k in ("Hon", "Htg", "act", "rew", "gam", "isw")]
    ws, ctr = be.iqn_workspace(B, 256, DEV), torch.tensor([F.CTR], device=DEV)
    a = _lib.IqnWideArgs()
    be._head_io(a.h.io, keep[0], keep[1], Pon, Ptg, *keep[2:], A, 512, 1.0 / B, td, loss, dH, dhead, None, None, None, None)
    Eon, Etg = {k: d(v) for k, v in fx["Eon"].items()}, {k: d(v) for k, v in fx["Etg"].items()}
    a.h.Eon, a.h.Etg, a.h.N, a.h.kappa, a.h.seed_q, a.h.ctr = be._embed(Eon), be._embed(Etg), N, 1.0, F.seed_q(), ctr.data_ptr()
    a.h.dpre, a.h.cosT, a.h.xg, a.h.gsum = (ws[k].data_ptr() for k in ("dpre", "cos", "xg", "gsum"))
    a.L = be.qr_wide_logits(3 * B, A, 256, DEV).data_ptr()
    if bad == "N":
        a.h.N = 257
    else:
        a.h.io.td_abs = None
    assert be.lib.apex_iqn_wide_head(a, _lib.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((td == -1).all()) and bool((loss == -1).all()) and bool((dhead == 7).all()) and not bool(dH.any())
    assert not bool(ws["dpre"].any()) and not bool(ws["xg"].any())


def _learner(cfg, backend="hip", split=False, seed=7, fill=11):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    torch.manual_seed(0)
    rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=seed)
    _fill_replay(rp, 1500, seed=fill)
    return FusedNatureLearner(cfg, DEV, rp, backend=backend, split=split), rp


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_iqn_wide_learner_step_hip_vs_torch_backend(dtype):
    """tests/test_gpu_iqn.py's whole-step test and bounds at N = 72 (stride 256, a second register set), B = 32."""
    from apex_dqn_amd.learner.iqn import iqn_seed, learner_taus
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, num_atoms=72, iqn_wide=True)
    res = {}
    for be in ("hip", "torch"):
        L, _ = _learner(cfg, be, split)
        assert L.N == 72 and L.iqn_wide and L.split == split and (L.qr_L is not None) == (be == "hip")
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        assert torch.equal(L.tau_out.cpu(), learner_taus(iqn_seed(cfg.Runtime.seed), 0, 32, 72))
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout)
    assert torch.equal(res["hip"][2], res["torch"][2])
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype}):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0 and float(gt["wtau"].norm()) > 0


def test_iqn_wide_graph_replays_are_bit_identical_to_eager():
    """A 4-update graph replayed twice leaves the bits of eight eager steps (no atomics, no host state in the draws)."""
    res = {}
    for graphs in (True, False):
        L, rp = _learner(_cfg(32, use_graphs=graphs, graph_steps=4, num_atoms=72, iqn_wide=True,
                              learner={"q_target_sync_freq": 1000}), seed=3, fill=1)
        if graphs:
            L.steps(8)
            assert L._multi is not None
        else:
            for _ in range(8):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 8 and L.iqn_wide
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.td_abs.clone(), L.tau_out.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
