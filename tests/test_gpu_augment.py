"""Random-shift (DrQ) frame augmentation on the GPU: csrc/augment.hip byte for byte against the
host mirror (learner/augment.py), the update index read on the device under graph replay, the
launcher's refusals, the whole step against the torch backend, graphs against eager steps,
resume and the GPU loop."""
import numpy as np
import pytest
import torch
from head_fixtures import fill_replay

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F_RING = 300
GUARD = 4096
CANARY = 0xA5
SEED, U0, BASE = 0, 5, 1000        # Runtime.seed, update index and counter base of the kernel tests
FRAME = 84 * 84


# --------------------------------------------------------------------- harness
@pytest.fixture(scope="module")
def ring():
    g = torch.Generator().manual_seed(42)
    return torch.randint(0, 256, (F_RING, 84, 84), dtype=torch.uint8, generator=g)


def _slots(rows, C, seed=0):
    """Random slots holding 0, F - 1, a slot repeated within a row and a slot shared by two rows
    (where the shape has room for them)."""
    g = torch.Generator().manual_seed(100 * rows + 10 * C + seed)
    s = torch.randint(0, F_RING, (rows, C), dtype=torch.int32, generator=g)
    flat = s.reshape(-1)
    flat[-1] = F_RING - 1
    if flat.numel() >= 2:
        flat[0] = 0
    if C >= 2 and rows >= 2:
        s[1, 1] = s[1, 0]                   # repeated within a row
    if rows >= 3:
        s[2, 0] = s[1, 0]                   # the same slot in two rows
    return s


def _guarded(n):
    buf = torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _mirror(ring, slots, P, u):
    """(out [rows C, 84, 84] in the ring's layout, offsets) by the mirror alone, on the CPU."""
    from apex_dqn_amd.learner import augment as AU
    from apex_dqn_amd.replay.gpu_replay import from_s2d, to_s2d
    rows, C = slots.shape
    off = AU.shift_offsets(AU.aug_seed(SEED), u, rows, P)
    nat = from_s2d(ring[slots.long()].reshape(rows * C, 84, 84)).reshape(rows, C, 84, 84)
    return to_s2d(AU.shift_frames(nat, off, P).reshape(rows * C, 84, 84)), off


def _launch(ops, ring_d, slots_d, P, ctr, base, out, off):
    from apex_dqn_amd.learner.augment import aug_seed
    ops.augment_shift(ring_d, slots_d, P, aug_seed(SEED), ctr, base, out, off)


# ------------------------------------------------------- 1. kernel vs the mirror
def test_the_chosen_draws_cover_every_offset():
    from apex_dqn_amd.learner import augment as AU
    sa = AU.aug_seed(SEED)
    o1 = AU.shift_offsets(sa, U0, 64, 1)
    assert {tuple(x) for x in o1.tolist()} == {(y, x) for y in range(3) for x in range(3)}
    o4 = AU.shift_offsets(sa, U0, 64, 4)
    for ax in (0, 1):
        assert int(o4[:, ax].min()) == 0 and int(o4[:, ax].max()) == 8


@pytest.mark.parametrize("rows,C,P", [(1, 1, 1), (5, 2, 4), (64, 4, 1), (64, 4, 4), (37, 4, 8)])
def test_augment_shift_kernel_vs_mirror(ring, rows, C, P):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    test_the_chosen_draws_cover_every_offset()
    slots = _slots(rows, C)
    want, want_off = _mirror(ring, slots, P, U0)
    ops = HipBackend()
    ring_d, slots_d = ring.to(DEV), slots.to(DEV)
    n = rows * C * FRAME
    buf, out = _guarded(n)
    off = torch.full((rows, 2), -7, dtype=torch.int32, device=DEV)
    ctr = torch.tensor([BASE + U0], dtype=torch.int64, device=DEV)
    base = torch.tensor([BASE], dtype=torch.int64, device=DEV)
    _launch(ops, ring_d, slots_d, P, ctr, base, out, off)
    torch.cuda.synchronize()
    assert torch.equal(off.cpu(), want_off)
    assert torch.equal(out.cpu().reshape(rows * C, 84, 84), want)
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + n:] == CANARY).all())
    assert torch.equal(ring_d.cpu(), ring) and torch.equal(slots_d.cpu(), slots)
    # no base word: u = the counter itself; a counter below the base clamps to update 0
    for ctr_v, base_t, u in ((3, None, 3), (BASE - 2, base, 0)):
        ctr.fill_(ctr_v)
        _launch(ops, ring_d, slots_d, P, ctr, base_t, out, off)
        torch.cuda.synchronize()
        w, wo = _mirror(ring, slots, P, u)
        assert torch.equal(off.cpu(), wo) and torch.equal(out.cpu().reshape(rows * C, 84, 84), w)
    # the torch backend (the oracle and the CPU path) writes the same buffer
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    out_t, off_t = torch.zeros(n, dtype=torch.uint8), torch.zeros(rows, 2, dtype=torch.int32)
    TorchBackend().augment_shift(ring, slots, P, _seed_a(), torch.tensor([BASE + U0]), torch.tensor([BASE]), out_t, off_t)
    assert torch.equal(out_t.reshape(rows * C, 84, 84), want) and torch.equal(off_t, want_off)


def _seed_a():
    from apex_dqn_amd.learner.augment import aug_seed
    return aug_seed(SEED)


# ------------------------------------------------ 2. u is read on the device
def test_update_index_is_read_inside_a_replayed_graph(ring):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    rows, C, P = 16, 4, 4
    slots = _slots(rows, C, seed=1)
    ops = HipBackend()
    ring_d, slots_d = ring.to(DEV), slots.to(DEV)
    n = rows * C * FRAME
    out = torch.zeros(n, dtype=torch.uint8, device=DEV)
    off = torch.zeros(rows, 2, dtype=torch.int32, device=DEV)
    out_e, off_e = torch.zeros_like(out), torch.zeros_like(off)
    ctr = torch.tensor([BASE + U0], dtype=torch.int64, device=DEV)
    base = torch.tensor([BASE], dtype=torch.int64, device=DEV)
    _launch(ops, ring_d, slots_d, P, ctr, base, out, off)          # (warm: module load outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(ops, ring_d, slots_d, P, ctr, base, out, off)
    seen = []
    for i in range(4):
        ctr.fill_(BASE + U0 + i)
        out.zero_()
        g.replay()
        _launch(ops, ring_d, slots_d, P, ctr, base, out_e, off_e)
        torch.cuda.synchronize()
        want, want_off = _mirror(ring, slots, P, U0 + i)
        assert torch.equal(off.cpu(), want_off), i
        assert torch.equal(off, off_e) and torch.equal(out, out_e), i
        assert torch.equal(out.cpu().reshape(rows * C, 84, 84), want), i
        seen.append(off.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[2], seen[3])


# ------------------------------------------------ 3. the launcher's refusals
def test_launcher_refusals(ring):
    from apex_dqn_amd.ops import _lib
    from apex_dqn_amd.ops.fused_ops import HipBackend
    rows, C, P = 4, 4, 4
    ops = HipBackend()
    ring_d, slots_d = ring.to(DEV), _slots(rows, C).to(DEV)
    n = rows * C * FRAME
    buf, out = _guarded(n)
    off = torch.full((rows, 2), -7, dtype=torch.int32, device=DEV)
    ctr = torch.tensor([BASE], dtype=torch.int64, device=DEV)
    base = torch.tensor([BASE], dtype=torch.int64, device=DEV)

    def args(**kw):
        a = ops.augment_args(ring_d, slots_d, P, _seed_a(), ctr, base, out, off)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    inside = ring_d.data_ptr() + 10 * FRAME
    bad = [dict(pad=0), dict(pad=9), dict(pad=-1), dict(C=3), dict(C=0), dict(C=8), dict(n_out=n - 1), dict(n_out=0),
           dict(out=inside), dict(out=ring_d.data_ptr()), dict(out=ring_d.data_ptr() + (F_RING - 1) * FRAME),
           dict(ring=None), dict(slots=None), dict(ctr=None), dict(out=None), dict(off_out=None), dict(rows=0),
           dict(F=0), dict(out=out.data_ptr() + 1)]
    for kw in bad:
        rc = ops.lib.apex_augment_shift(args(**kw), _lib.stream_ptr())
        assert rc != 0, kw
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and bool((off == -7).all())          # nothing was launched
    assert torch.equal(ring_d.cpu(), ring)
    with pytest.raises(RuntimeError, match="augment_shift"):
        _lib.check(ops.lib.apex_augment_shift(args(pad=9), _lib.stream_ptr()), "augment_shift")
    # the unaltered block launches
    assert ops.lib.apex_augment_shift(args(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((off >= 0).all()) and bool((off <= 2 * P).all()) and not bool((out == CANARY).all())


# -------------------------------------------------------------- 4. whole step
def _cfg(B, **rt):
    from apex_dqn_amd.config import ApexConfig
    learner = rt.pop("learner", {})
    return ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "Synthetic"},
                                 "Learner": {"replay_sample_size": B, **learner},
                                 "Runtime": {"augment_shift": 4, **rt}})


@pytest.mark.parametrize("dtype,rt", [("bf16", {}), ("fp32", {}), ("fp32", dict(num_atoms=32, dist_head="quantile")),
                                      ("fp32", dict(munchausen=True))])
def test_augmented_learner_step_hip_vs_torch_backend(dtype, rt):
    """tests/test_gpu_noisy.py test_noisy_learner_step_hip_vs_torch_backend with the shift on: both backends read
    identical augmented bytes, so that test's bounds on td_abs, loss_b and the per-segment gradient errors and
    its clip-norm identity hold unchanged."""
    from apex_dqn_amd.learner import augment as AU
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    split = dtype == "fp32"
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, **rt)
    res = {}
    for be in ("hip", "torch"):
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=7)
        fill_replay(rp, 1500, seed=11)
        L = FusedNatureLearner(cfg, DEV, rp, backend=be, split=split)
        assert L.aug_pad == 4 and L.split == split and L.munchausen == bool(rt.get("munchausen"))
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        gn = float(L.g32.double().norm()) * L.is_scale()
        assert abs(float(L.gnorm) - gn) <= 1e-5 * gn, (be, float(L.gnorm), gn)
        res[be] = (L.td_abs.clone(), L.g32.clone(), L.S["idx"].clone(), L.loss_b.clone(), L.layout,
                   L.aug_frames.clone(), L.aug_off.clone(), L.slots.clone())
    assert torch.equal(res["hip"][2], res["torch"][2]) and torch.equal(res["hip"][7], res["torch"][7])
    assert torch.equal(res["hip"][5], res["torch"][5]) and torch.equal(res["hip"][6], res["torch"][6])
    off = AU.shift_offsets(AU.aug_seed(cfg.Runtime.seed), 0, 64, 4)
    assert torch.equal(res["hip"][6].cpu(), off) and float((off - 4).abs().max()) > 0
    torch.testing.assert_close(res["hip"][0], res["torch"][0], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(res["hip"][3], res["torch"][3], rtol=5e-2, atol=5e-2)
    lay = res["hip"][4]
    gh, gt = lay.views(res["hip"][1]), lay.views(res["torch"][1])
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype} HIP step vs the torch backend, {rt}):", errs)
    assert max(errs.values()) < 0.2, errs
    assert float(gt["wv"].norm()) > 0 and float(gt["wa"].norm()) > 0 and float(gt["w1"].norm()) > 0


# ------------------------------------------------------------------ 5. graphs
def test_augmented_graph_steps_match_eager_steps():
    """steps(8) replaying two 4-update graphs == 8 eager step() calls of a twin at P = 4, at
    tests/test_gpu_noisy.py's tolerances; the offsets left on the device are the mirror's for update 7: the
    index is read inside the replayed graph."""
    from apex_dqn_amd.learner import augment as AU
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    res = {}
    for graphs in (True, False):
        cfg = _cfg(64, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000})
        torch.manual_seed(0)
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=3)
        fill_replay(rp, 1500, seed=1)
        L = FusedNatureLearner(cfg, DEV, rp, backend="hip")
        u0 = L.update_index()
        if graphs:
            L.steps(8)
            assert L._multi is not None
        else:
            for _ in range(8):
                L.step()
        torch.cuda.synchronize()
        assert L.num_q_updates == 8 and L.update_index() - u0 == 8
        assert torch.equal(L.aug_off.cpu(), AU.shift_offsets(AU.aug_seed(cfg.Runtime.seed), 7, 128, 4)), graphs
        off, frames = L.aug_off.clone(), L.aug_frames.clone()
        if graphs:
            assert L.graph_matches_eager() is True
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.S["idx"].clone(), off, frames)
    assert torch.equal(res[True][3], res[False][3])
    assert torch.equal(res[True][4], res[False][4])                  # the same offsets, bit for bit
    for a, b in zip(res[True][:3], res[False][:3]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


# -------------------------------------------------------- 6. resume, GPU loop
def test_augmented_resume_matches_uninterrupted_run(tmp_path):
    """Save after 4 updates, load into a fresh learner, 4 more: bit-equal to 8 uninterrupted updates -- the
    shifts continue at the restored update index."""
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard

    def replay():
        rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=5)
        fill_replay(rp, 1500, seed=2)
        return rp

    cfg = _cfg(32, use_graphs=True, learner={"q_target_sync_freq": 3})
    rp = replay()
    torch.manual_seed(0)
    L = FusedNatureLearner(cfg, DEV, rp)
    for _ in range(4):
        L.step()
    torch.cuda.synchronize()
    ck = str(tmp_path / "ck.pt")
    L.save(ck)
    tree = [t.clone() for t in (rp.leaf, rp.nodes, rp.min_bits, rp.ctr)]
    for _ in range(4):
        L.step()
    torch.cuda.synchronize()
    rp2 = replay()
    for dst, src in zip((rp2.leaf, rp2.nodes, rp2.min_bits, rp2.ctr), tree):
        dst.copy_(src)
    d = cfg.to_dict()
    torch.manual_seed(9)
    L2 = FusedNatureLearner(ApexConfig.from_dict({**d, "Learner": {**d["Learner"], "load_saved_state": ck}}), DEV, rp2)
    assert L2.aug_pad == 4 and L2.num_q_updates == L2.update_index() == 4
    for _ in range(4):
        L2.step()
    torch.cuda.synchronize()
    for a, b in ((L.p32, L2.p32), (L.rms_v, L2.rms_v), (L.rms_m, L2.rms_m), (L.t32, L2.t32), (rp.leaf, rp2.leaf),
                 (rp.ctr, rp2.ctr), (L.S["weights"], L2.S["weights"]), (L.aug_off, L2.aug_off),
                 (L.aug_frames, L2.aug_frames)):
        assert torch.equal(a, b)


def test_augmented_gpu_loop_lock_step_on_fake_ale():
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.runtime.gpu_loop import train_frames
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "PongNoFrameskip-v4"},
                                "Actor": {"num_actors": 16, "n_step_transition_batch_size": 16,
                                          "Q_network_sync_freq": 10},
                                "Learner": {"min_replay_mem_size": 300, "replay_sample_size": 32,
                                            "remove_old_xp_freq": 8, "q_target_sync_freq": 5},
                                "Replay_Memory": {"soft_capacity": 4000},
                                "Runtime": {"log_every": 8, "use_graphs": True, "graph_steps": 4,
                                            "env_backend": "fake_ale", "augment_shift": 4}})
    out = train_frames(cfg, DEV, 16, num_envs=16, async_actors=False)
    L = out["learner"]
    torch.cuda.synchronize()
    assert L.aug_pad == 4 and L.num_q_updates == L.update_index() == 16
    assert bool(torch.isfinite(L.td_abs).all()) and float(L.td_abs.max()) > 0
    m = L.last_metrics()
    assert np.isfinite(m["loss"]) and m["grad_norm"] > 0
    assert 0 <= m["augment_offset_mean"] <= 8 and m["augment_offset_mean"] == float(L.aug_off.double().mean())
    assert int(L.aug_off.min()) >= 0 and int(L.aug_off.max()) <= 8
