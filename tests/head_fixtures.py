"""Helpers the head test files share: the hi / lo planes of fp32 activations (tests/ddqn_fixtures.py's) and
the synthetic replay fill of the whole-step tests."""
import numpy as np
from ddqn_fixtures import split_planes  # noqa: F401


def fill_replay(rp, K, A=6, seed=0):
    rng = np.random.default_rng(seed)
    seqs = rp.append_frames(rng.integers(0, 255, (K + 8, 84, 84), dtype=np.uint8))
    st = np.stack([seqs[i:i + 4] for i in range(K)])
    rp.insert(dict(S_t=st, S_tpn=st + 3, A_t=rng.integers(0, A, K), R=rng.normal(size=K).astype(np.float32),
                   Gamma=np.where(rng.random(K) < 0.1, 0.0, 0.97).astype(np.float32),
                   priority=rng.random(K).astype(np.float32) * 3 + 0.01))
