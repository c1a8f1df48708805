"""The device exploration draw of include/simaps_action_as.h, restated with Python ints and NumPy:
Philox4x32-10 (Salmon et al., SC'11) and the two values taken from its output."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words -> the 4 output words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw(seed, step, n, eps, total):
    """Agent n of a call at (seed, step): (explored, action); action is -1 when it does not explore."""
    w = philox4x32_10((n, 0, step & MASK, step >> 32), (seed & MASK, seed >> 32))
    u = np.float32(w[0] >> 8) * np.float32(2.0 ** -24)
    if u < np.float32(eps):
        return True, (w[1] * int(total)) >> 32
    return False, -1


def draws(seed, step, n_agents, eps, totals):
    """draw() for agents 0..n_agents-1; eps and totals scalars or per agent -> (explored bool [n], action int64 [n])."""
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float32), (n_agents,))
    totals = np.broadcast_to(np.asarray(totals, dtype=np.int64), (n_agents,))
    out = [draw(seed, step, n, eps[n], totals[n]) for n in range(n_agents)]
    return np.array([o[0] for o in out], dtype=bool), np.array([o[1] for o in out], dtype=np.int64)
