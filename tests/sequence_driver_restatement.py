"""What tools/make_golden_sequence_drivers.py and tests/test_gpu_sequence_drivers.py share: the seeded synthetic data and
sample orders of the epoch fixtures G21 / G22 (the fixtures keep seeds and sums, not the arrays)."""
import numpy as np


def synthetic_u(seed, trajectories):
    """[S, 64, 64, 20] float32: seeded fields of unit scale (a random field that decays in time plus fresh noise per frame)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((trajectories, 64, 64, 1)).astype(np.float32)
    return (base * np.linspace(1.0, 0.5, 20, dtype=np.float32) + 0.3 * rng.standard_normal((trajectories, 64, 64, 20))).astype(np.float32)


def permutations(seed, epochs, n):
    rng = np.random.default_rng(seed)
    return [rng.permutation(n).tolist() for _ in range(epochs)]
