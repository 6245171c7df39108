"""Device-side Atari preprocessing on the GPU: csrc/atari_frames.hip (max of the raw frame pair,
gray, area resize, rounding, s2d permutation, ring scatter) against its host mirror
``atari_preprocess_exact`` -- integer arithmetic with one right answer, so every comparison is
bit for bit -- then the replay's raw append from its pinned staging buffers and an actor group
in device mode."""
import numpy as np
import pytest
import torch

from apex_dqn_amd.envs.vector_envs import RAW_FRAME_SHAPE, atari_preprocess_exact, make_vec_env
from apex_dqn_amd.ops import _lib
from apex_dqn_amd.replay.gpu_replay import GpuReplayShard, from_s2d

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FILL = 0xA5


def _run(raw: np.ndarray, F: int, start: int, n=None):
    """The kernel on ``raw`` into a ring of F slots pre-filled with FILL; the ring on the host."""
    lib = _lib.require_kernels()
    d_raw = torch.from_numpy(raw).to(DEV)
    ring = torch.full((F, 84, 84), FILL, dtype=torch.uint8, device=DEV)
    rc = lib.apex_atari_frames(d_raw.data_ptr(), ring.data_ptr(), raw.shape[0] if n is None else n, F, start,
                               _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, ring.cpu()


def _gray(plane: np.ndarray) -> np.ndarray:
    return np.repeat(plane.astype(np.uint8)[:, :, None], 3, axis=2)


def test_kernel_matches_mirror_with_ring_wrap():
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 256, (3,) + RAW_FRAME_SHAPE, dtype=np.uint8)
    rc, ring = _run(raw, F=5, start=3)                 # frames land in slots 3, 4, 0
    assert rc == 0
    got = from_s2d(ring[[3, 4, 0]]).numpy()
    np.testing.assert_array_equal(got, atari_preprocess_exact(raw))
    assert (ring[1:3] == FILL).all()                   # the other slots are untouched


def test_kernel_ties_constants_and_max():
    def pair(plane):
        return np.stack([_gray(plane)] * 2)

    tie20 = np.zeros((210, 160), np.uint8)
    tie20[:, 1] = 20                                   # output column 0 = 9.5 -> 10
    tie60 = np.zeros((210, 160), np.uint8)
    tie60[:, 1] = 60                                   # 28.5 -> 28
    white = np.full((210, 160), 255, np.uint8)
    black = np.zeros((210, 160), np.uint8)
    # only frame 0 is bright in one region and only frame 1 in another (colour, not gray)
    rng = np.random.default_rng(1)
    f0 = rng.integers(0, 40, (210, 160, 3), dtype=np.uint8)
    f1 = rng.integers(0, 40, (210, 160, 3), dtype=np.uint8)
    f0[20:70, 10:90] = (250, 200, 230)
    f1[120:205, 70:158] = (180, 255, 90)
    raw = np.stack([pair(tie20), pair(tie60), pair(white), pair(black), np.stack([f0, f1])])
    rc, ring = _run(raw, F=5, start=0)
    assert rc == 0
    got = from_s2d(ring).numpy()
    assert (got[0][:, 0] == 10).all() and (got[1][:, 0] == 28).all()
    assert (got[2] == 255).all() and (got[3] == 0).all()
    assert got[4][8:28, 6:46].min() > 150 and got[4][48:82, 38:82].min() > 150    # both regions made it
    np.testing.assert_array_equal(got, atari_preprocess_exact(raw))


def test_kernel_argument_checks_launch_nothing():
    raw = np.zeros((1,) + RAW_FRAME_SHAPE, np.uint8)
    rc, ring = _run(raw, F=3, start=0, n=0)
    assert rc == 0 and (ring == FILL).all()
    lib = _lib.require_kernels()
    d_raw = torch.zeros(2 * int(np.prod(RAW_FRAME_SHAPE)), dtype=torch.uint8, device=DEV)
    d_ring = torch.full((2 * 7056,), FILL, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(DEV)
    invalid = 1                                        # hipErrorInvalidValue
    assert lib.apex_atari_frames(d_raw.data_ptr() + 4, d_ring.data_ptr(), 1, 1, 0, st) == invalid
    assert lib.apex_atari_frames(d_raw.data_ptr(), d_ring.data_ptr() + 8, 1, 1, 0, st) == invalid
    assert lib.apex_atari_frames(d_raw.data_ptr(), d_ring.data_ptr(), 2, 1, 0, st) == invalid   # n > F
    assert lib.apex_atari_frames(d_raw.data_ptr(), d_ring.data_ptr(), 1, 2, 2, st) == invalid   # start >= F
    torch.cuda.synchronize()
    assert (d_ring == FILL).all()


def test_replay_raw_append_from_staging_equals_copied_append():
    n, F = 4, 6
    a = GpuReplayShard(64, 64, F, 4, device=DEV)
    b = GpuReplayShard(64, 64, F, 4, device=DEV)
    rng = np.random.default_rng(3)
    bufs, frames = [], []
    for _ in range(5):                                 # both pinned buffers, several wraps
        raw = rng.integers(0, 256, (n,) + RAW_FRAME_SHAPE, dtype=np.uint8)
        buf = a.stage_frames(n, raw=True)
        assert buf.shape == (n,) + RAW_FRAME_SHAPE and buf.dtype == np.uint8
        bufs.append(buf)
        buf[...] = raw
        sa = a.append_raw_frames(buf)
        sb = b.append_raw_frames(raw.copy())
        np.testing.assert_array_equal(sa, sb)
        frames.append(atari_preprocess_exact(raw))
        torch.cuda.synchronize()
        assert torch.equal(a.frames, b.frames)
    assert not np.shares_memory(bufs[0], bufs[1])
    assert np.shares_memory(bufs[0], bufs[2]) and np.shares_memory(bufs[1], bufs[3])
    assert a.frame_head == b.frame_head == 5 * n
    want = np.concatenate(frames)                      # seq s lives in slot s % F; the newest F survive
    seqs = np.arange(5 * n - F, 5 * n)
    got = from_s2d(a.frames[torch.from_numpy(seqs % F).to(DEV)]).cpu().numpy()
    np.testing.assert_array_equal(got, want[seqs])
    # more pairs than ring slots in one append: only the newest F are stored
    raw = rng.integers(0, 256, (F + 2,) + RAW_FRAME_SHAPE, dtype=np.uint8)
    s = a.append_raw_frames(raw)
    torch.cuda.synchronize()
    keep = s[2:]
    got = from_s2d(a.frames[torch.from_numpy(keep % F).to(DEV)]).cpu().numpy()
    np.testing.assert_array_equal(got, atari_preprocess_exact(raw[2:]))


def test_actor_group_device_mode_fills_the_ring_with_mirror_frames():
    from apex_dqn_amd.actors.gpu_actor import GpuActorGroup, make_gpu_actor_group
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    E, steps = 4, 6
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": 6, "name": "PongNoFrameskip-v4"},
                                "Actor": {"num_actors": E, "n_step_transition_batch_size": 4, "num_steps": 3},
                                "Learner": {"replay_sample_size": 16},
                                "Runtime": {"use_graphs": False, "env_backend": "fake_ale",
                                            "atari_preprocess": "device"}})
    torch.manual_seed(3)
    rp = GpuReplayShard(256, 256, 64, 4, device=DEV)
    L = FusedNatureLearner(cfg, DEV, rp)
    grp = make_gpu_actor_group(cfg, L, rp, E)
    assert type(grp) is GpuActorGroup and grp.env.raw_frames
    recorded = []
    env_step = grp.env.step

    def recording_step(actions, out=None):
        recorded.append(np.array(actions))
        return env_step(actions, out=out)

    grp.env.step = recording_step
    inserted = sum(grp.step() for _ in range(steps))
    torch.cuda.synchronize()
    assert len(recorded) == steps and inserted == grp.inserted > 0 and rp.size() == inserted
    twin = make_vec_env("fake_ale", "PongNoFrameskip-v4", E, 6, seed=0, preprocess="device")
    raws = [twin.reset()] + [twin.step(a)[0] for a in recorded]
    want = atari_preprocess_exact(np.concatenate(raws))          # frame seq = step * E + env
    assert rp.frame_head == (steps + 1) * E == want.shape[0]
    got = from_s2d(rp.frames[:want.shape[0]]).cpu().numpy()
    np.testing.assert_array_equal(got, want)
