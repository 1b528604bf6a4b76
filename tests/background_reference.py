"""Reference for the Markov backgrounds (crbm_amd/background.py, crbm_amd/csrc/crbm_background.h), NumPy on the host and
written independently of both: a j-mer counter over explicit windows and a validity cumsum, and a plain sequential
sampler over oracle.crbm_oracle.philox4x32 that follows the contract of include/crbm_amd.h (crbm_background_sample)
literally.  Shared by the CPU, emulation and GPU tests; nothing here is ever written to by a test."""
import numpy as np

from oracle.crbm_oracle import philox4x32

KIND_BACKGROUND = 8
M32 = 2 ** 32 - 1


def contexts(order):
    return sum(4 ** j for j in range(order + 1))


def context_index(letters):
    """(4^j - 1) / 3 + sum_i l_i 4^(j - i) for the letters l_1 .. l_j, oldest first"""
    j = len(letters)
    return (4 ** j - 1) // 3 + sum(int(l) * 4 ** (j - 1 - i) for i, l in enumerate(letters))


def kmer_counts(codes, order):
    """uint64 counts of the j-mers, j = 1 .. order + 1, back to back, the oldest letter most significant: position p
    counts for j when codes[p .. p + j) are all letters"""
    codes = np.asarray(codes, np.uint8)
    T = codes.size
    letter = (codes < 4).astype(np.int64)
    before = np.concatenate([[0], np.cumsum(letter)])            # letters in codes[:p]
    out = []
    for j in range(1, order + 2):
        counts = np.zeros(4 ** j, np.uint64)
        if T >= j:
            p = np.arange(T - j + 1)
            ok = before[p + j] - before[p] == j
            idx = np.zeros(T - j + 1, np.int64)
            for i in range(j):
                idx = idx * 4 + np.where(ok, codes[i:T - j + 1 + i].astype(np.int64), 0)
            counts += np.bincount(idx[ok], minlength=4 ** j).astype(np.uint64)
        out.append(counts)
    return np.concatenate(out)


def draws(seed, pos0, T):
    """u_p for P = pos0 .. pos0 + T - 1: word (P & 3) of philox4x32((uint32)(P >> 2), (uint32)(P >> 34), 8 << 28, 0, seed)"""
    if T == 0:
        return np.zeros(0, np.uint32)
    P = np.arange(pos0, pos0 + T, dtype=np.uint64)
    block = P >> np.uint64(2)                                    # (block >> 32 is P >> 34)
    first, last = int(block[0]), int(block[-1])
    b = np.arange(first, last + 1, dtype=np.uint64)
    r = philox4x32(b & np.uint64(M32), (b >> np.uint64(32)) & np.uint64(M32), np.uint64(KIND_BACKGROUND << 28), np.uint64(0),
                   np.uint64(seed & M32), np.uint64((seed >> 32) & M32))
    words = np.stack([np.asarray(w, np.uint64) for w in r], axis=1).reshape(-1)      # block-major, word-minor
    return words[(P - np.uint64(4 * first)).astype(np.int64)].astype(np.uint32)


def sample(table, order, template, seed, pos0=0):
    """the contract, one position after the other.  template: a uint8 stream or an integer length"""
    table = np.asarray(table, np.uint32)
    assert table.shape == (contexts(order), 3)
    tmpl = np.zeros(template, np.uint8) if isinstance(template, (int, np.integer)) else np.asarray(template, np.uint8)
    T = tmpl.size
    u = draws(int(seed) & (2 ** 64 - 1), pos0, T)
    rows = [[int(x) for x in row] for row in table]
    out = np.empty(T, np.uint8)
    ctx = []                                                     # the last <= order letters, oldest first
    for p in range(T):
        if tmpl[p] == 4:
            out[p] = 4
            ctx = []
            continue
        row = rows[context_index(ctx)]
        up = int(u[p])
        a = (up >= row[0]) + (up >= row[1]) + (up >= row[2])
        out[p] = a
        ctx = (ctx + [a])[-order:] if order else []
    return out


def thresholds_from_probabilities(P):
    """thr[ctx][i] = min(2^32 - 1, floor(2^32 sum_{a <= i} P[ctx][a])) for P (contexts, 4) float64"""
    cum = np.cumsum(np.asarray(P, np.float64)[:, :3], axis=1)
    return np.minimum(np.floor(cum * 2.0 ** 32), float(M32)).astype(np.uint32)


def probabilities_of(table):
    """(contexts, 4) float64: the exact probability of every letter under a threshold table (u uniform on 0 .. 2^32 - 1)"""
    t = np.asarray(table, np.float64)
    edges = np.concatenate([np.zeros((t.shape[0], 1)), t, np.full((t.shape[0], 1), 2.0 ** 32)], axis=1)
    return np.diff(edges, axis=1) / 2.0 ** 32


def dirichlet_table(order, seed, alpha=0.3):
    rng = np.random.default_rng(seed)
    return thresholds_from_probabilities(rng.dirichlet(np.full(4, alpha), size=contexts(order)))


def rotation_table():
    """order 1: a' = (a + 1) mod 4 whatever the draw; the empty context draws a letter uniformly.  Chains from different
    letters never meet."""
    M = M32
    return np.array([[2 ** 30, 2 ** 31, 3 * 2 ** 30], [0, M, M], [0, 0, M], [0, 0, 0], [M, M, M]], np.uint32)


def stuck_table(order=3):
    """rows [0, 0, 0] (always T) and [M, M, M] (always A, but for u = 2^32 - 1) alternating by context index, the empty
    context uniform: nothing coalesces by chance, the chain is a function of its context alone"""
    t = np.zeros((contexts(order), 3), np.uint32)
    t[1::2] = M32
    t[0] = [2 ** 30, 2 ** 31, 3 * 2 ** 30]
    return t


def gapped_stream(T, seed, gap_share=0.02, max_run=6):
    """letters with runs of gaps, about gap_share of the positions"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, T).astype(np.uint8)
    n = max(1, int(T * gap_share / ((1 + max_run) / 2.0)))
    for at, ln in zip(rng.integers(0, max(T, 1), n), rng.integers(1, max_run + 1, n)):
        s[at:at + ln] = 4
    return s
