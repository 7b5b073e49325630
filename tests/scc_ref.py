"""The reference of the strongly-connected-components tests (bspgemm_strongly_connected_components): scipy's strong
components, relabelled to the smallest vertex id of every component, and the small directed graphs the tests use beside
those of cc_ref.py.  Row u of a graph lists the out-neighbours of u.  Nothing here touches the GPU.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

from cc_ref import K_SEL_STAGE, K_SEL_TILE, csr, cycle, members, path, path_permuted, sparse_far_rows, star  # noqa: F401


def labels(rp, ci, n):
    """(label int32[n], ncomponents): label[v] = the smallest vertex id of v's strongly connected component"""
    if n == 0:
        return np.zeros(0, np.int32), 0
    ci = np.asarray(ci)
    G = csr_matrix((np.ones(ci.size), ci.copy(), np.asarray(rp).copy()), shape=(n, n))
    G.sum_duplicates()      # canonical first: on a CSR with repeated entries scipy's strong components may not return
    G.sort_indices()
    ncomp, comp = connected_components(G, directed=True, connection="strong")
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.int32), int(ncomp)


def largest(label):
    """the size of the largest component"""
    return int(np.bincount(label).max()) if label.size else 0


def transposed(rp, ci, n):
    """the same graph with every entry reversed, rows ascending"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    return csr(ci, rows, n)


# ---------------------------------------------------------------- graphs ---------------------------------------------
def cycle_reversed(n):
    """v -> v - 1 (mod n): one cycle whose colour travels against the id order"""
    return csr(np.arange(n), (np.arange(n) - 1) % n, n)


def two_cycles(k, entry):
    """the cycles 0 .. k - 1 and k .. 2k - 1 joined by ONE entry: "down" from the lower-id cycle into the higher one (the
    higher cycle takes the lower one's colour), "up" the other way"""
    a = np.arange(k)
    rows, cols = np.concatenate([a, k + a]), np.concatenate([(a + 1) % k, k + (a + 1) % k])
    u, v = k // 5, k + k // 5
    if entry == "up":
        u, v = v, u
    return csr(np.append(rows, u), np.append(cols, v), 2 * k)


def ladder(k, entry):
    """k two-cycles {2i, 2i + 1} chained by one entry each: "down" 2i + 1 -> 2i + 2 (every two-cycle below the first is
    reached from all before it: one SCC per colouring round), "up" 2i + 2 -> 2i + 1 (every two-cycle keeps its own colour)"""
    i = np.arange(k)
    j = np.arange(k - 1)
    link = (2 * j + 1, 2 * j + 2) if entry == "down" else (2 * j + 2, 2 * j + 1)
    return csr(np.concatenate([2 * i, 2 * i + 1, link[0]]), np.concatenate([2 * i + 1, 2 * i, link[1]]), 2 * k)


def tails(tail=20, ring=30):
    """a path of `tail` vertices into a cycle of `ring`, a path of `tail` vertices out of it, and a last vertex with a
    self-loop and one in-edge from the end of that path: only the cycle survives trimming, which takes `tail` passes and
    more (every pass exposes the next vertex), and the self-loop counts for nothing.  tail + tail + 2 components."""
    n = 2 * tail + ring + 1
    t_in, c, t_out = np.arange(tail), tail + np.arange(ring), tail + ring + np.arange(tail)
    rows = np.concatenate([t_in, c, [c[-1]], t_out[:-1], [t_out[-1]], [n - 1]])
    cols = np.concatenate([t_in + 1, tail + (np.arange(ring) + 1) % ring, [t_out[0]], t_out[1:], [n - 1], [n - 1]])
    return csr(rows, cols, n)


def four_cycles(entries, seed):
    """exactly `entries` stored entries as a union of directed 4-cycles over shuffled ids (the remainder: one cycle of 2, 3
    or 5, never a self-loop), and isolated vertices up to an n that is no multiple of 4"""
    rng = np.random.default_rng(seed)
    full, rest = divmod(entries, 4)
    lengths = [4] * full + ([rest] if rest >= 2 else [])
    if rest == 1:
        lengths[-1] = 5
    n = sum(lengths) + 7
    n += n % 4 == 0
    ids = rng.permutation(n)
    rows, cols, at = [], [], 0
    for k in lengths:
        c = ids[at:at + k]
        rows.append(c)
        cols.append(np.roll(c, -1))
        at += k
    return csr(np.concatenate(rows), np.concatenate(cols), n) + (lengths,)


def star_both(n, hub):
    """the star stored in both directions, hub -> leaf and leaf -> hub: 2 (n - 1) entries, one component"""
    leaves = np.setdiff1d(np.arange(n), [hub])
    return csr(np.concatenate([np.full(n - 1, hub), leaves]), np.concatenate([leaves, np.full(n - 1, hub)]), n)


def three_cycles(n):
    """v -> v + 3, the last vertex of every residue class back to its first: exactly three interleaved cycles"""
    v = np.arange(n)
    return csr(v, np.where(v + 3 < n, v + 3, v % 3), n)


def untidy(n, seed):
    """about 2 n random directed edges among n vertices (a large component and many small ones), 30 % of them stored twice,
    a self-loop on every fifth vertex, the entries of every row in shuffled order"""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, size=(2, 2 * n))
    again = rng.random(r.size) < 0.3
    loops = np.arange(0, n, 5)
    rows, cols = np.concatenate([r, r[again], loops]), np.concatenate([c, c[again], loops])
    o = rng.permutation(rows.size)
    return csr(rows[o], cols[o], n)
