"""The reference of the maximal-matching tests (bspgemm_maximal_matching): the edge key formula of include/bspgemm.h, plain
sequential greedy over the sorted edges (the definition), a numpy model of the rounds as the library runs them (the
locally-dominant-edge algorithm) that also predicts the counts of bspgemm_match_info, the properties of a maximal
matching, and the graphs the tests use.  Nothing here touches the GPU.
"""
import collections

import numpy as np

import cc_ref
import color_ref
import kcore_ref
from color_ref import mix32
from kcore_ref import simple

ORDERS = ("natural", "random", "light")
LANES = (0, 4, 16, 64)   # BSPGEMM_OPT_MATCH_LANES
CHUNK = 4096             # csrc/match.hip kMatchChunk: the longest row left to one group of lanes, and the entries of a chunk
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)

Matching = collections.namedtuple("Matching", "mate labels pairs rounds entries_walked hub_chunks lanes")


def edge_keys(a, b, order, seed, deg):
    """key32 uint32 of the edges {a, b}, a < b elementwise.  deg: the degrees in simple(A)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    assert (a < b).all()
    if order == "natural":
        return np.zeros(a.shape, np.uint32)
    h = mix32(mix32(a.astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)) ^ b.astype(np.uint32))
    if order == "random":
        return h
    assert order == "light", order
    deg = np.asarray(deg, np.int64)
    weight = np.minimum(deg[a] + deg[b], 0xffff).astype(np.uint32)
    return (weight << np.uint32(16)) | (h >> np.uint32(16))


def edges_of(srp, sci, n):
    """(a, b) of the edges of a simple graph, a < b, in row order"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(srp))
    up = rows < sci
    return rows[up], sci[up].astype(np.int64)


def greedy(srp, sci, n, order="random", seed=0):
    """mate int32[n] of plain sequential greedy: the edges sorted by (key32, a, b), an edge is taken when both ends are free"""
    a, b = edges_of(srp, sci, n)
    key = edge_keys(a, b, order, seed, np.diff(srp))
    mate = np.full(n, -1, np.int32)
    for i in np.lexsort((b, a, key)).tolist():
        if mate[a[i]] < 0 and mate[b[i]] < 0:
            mate[a[i]], mate[b[i]] = b[i], a[i]
    return mate


def chunks_of(deg, chunk=CHUNK):
    """the chunk records of rows of `deg` entries: none for a row that a group of lanes walks itself"""
    deg = np.asarray(deg, np.int64)
    return np.where(deg > chunk, (deg + chunk - 1) // chunk, 0)


def lanes_for(entries, listed, forced=0):
    """the lanes per live vertex: forced, or the smallest of 4, 16, 64 at or above a quarter of the mean degree of the
    vertices that have one (0 without a round)"""
    if listed == 0:
        return 0
    if forced:
        return forced
    if entries <= 16 * listed:
        return 4
    return 16 if entries <= 64 * listed else 64


def matching_of(srp, sci, n, order="random", seed=0, chunk=CHUNK, lanes=0):
    """the round model on a simple graph: a Matching"""
    deg = np.diff(srp).astype(np.int64)
    mate = np.full(n, -1, np.int64)
    live = np.flatnonzero(deg > 0)
    pairs = rounds = walked = hubs = 0
    width = lanes_for(int(sci.size), int(live.size), lanes)
    while live.size:
        rounds += 1
        assert rounds <= n
        walked += int(deg[live].sum())
        hubs += int(chunks_of(deg[live], chunk).sum())
        owner, nb = color_ref._rows_with_owner(srp, sci, live)
        u, nb = live[owner], nb.astype(np.int64)
        cand = (edge_keys(np.minimum(u, nb), np.maximum(u, nb), order, seed, deg).astype(np.uint64) << np.uint64(32)) | nb.astype(np.uint64)
        cand[mate[nb] >= 0] = NONE
        best = np.full(n, NONE, np.uint64)
        start = np.concatenate([[0], np.cumsum(deg[live])[:-1]])       # every live row has entries
        best[live] = np.minimum.reduceat(cand, start)
        mine = best[live]
        has = mine != NONE
        w = (mine & np.uint64(0xFFFFFFFF)).astype(np.int64)
        w[~has] = 0
        back = has & ((best[w] & np.uint64(0xFFFFFFFF)).astype(np.int64) == live) & (best[w] != NONE)
        mate[live[back]] = w[back]
        pairs += int((back & (live < w)).sum())
        live = live[has & ~back]
    v = np.arange(n, dtype=np.int64)
    labels = np.where(mate >= 0, np.minimum(v, mate), v).astype(np.int32)
    return Matching(mate.astype(np.int32), labels, pairs, rounds, walked, hubs, width)


def matching(rp, ci, n, order="random", seed=0, chunk=CHUNK, lanes=0):
    """the Matching that bspgemm_maximal_matching defines for the graph of A's entries: mate (-1 = unmatched), labels =
    P.col_idx, and the counts of bspgemm_match_info"""
    srp, sci = simple(rp, ci, n)
    return matching_of(srp, sci, n, order, seed, chunk, lanes)


def check_properties(srp, sci, n, mate):
    """symmetric mates, every pair is an edge of S, and no edge of S has two free ends"""
    mate = np.asarray(mate, np.int64)
    assert mate.shape == (n,)
    m = np.flatnonzero(mate >= 0)
    assert (mate[m] < n).all() and (mate[m] != m).all() and np.array_equal(mate[mate[m]], m), "mates are not symmetric"
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(srp))
    stored = set((rows * np.int64(n + 1) + sci).tolist())
    assert all(int(v) * (n + 1) + int(mate[v]) in stored for v in m), "a pair is no edge of S"
    assert not ((mate[rows] < 0) & (mate[sci] < 0)).any(), "an edge of S has two free ends"


# ---------------------------------------------------------------- graphs ---------------------------------------------
def star_hub_last(leaves):
    """leaves 0 .. leaves - 1 joined to the hub `leaves`: the position of a leaf in the hub's row is its id"""
    return cc_ref.star(leaves + 1, leaves, "hub")


def two_hubs(leaves):
    """two stars of `leaves` leaves each whose hubs (the two last ids) are adjacent"""
    h0, h1 = 2 * leaves, 2 * leaves + 1
    rows = np.concatenate([np.full(leaves, h0), np.full(leaves, h1), [h0]])
    cols = np.concatenate([np.arange(leaves), np.arange(leaves, 2 * leaves), [h1]])
    return cc_ref.csr(rows, cols, 2 * leaves + 2)


def hub_live3(k):
    """a hub 4k with the leaves l_i = 3k + i, each leaf with a pendant path l_i - p_i - q_i - r_i (p_i = 2k + i, q_i = k + i,
    r_i = i).  Under NATURAL the edges further from the hub come first: round 1 matches q_i - r_i, round 2 p_i - l_i, and
    in round 3 the hub, live since round 1, has no free neighbour left and retires"""
    i = np.arange(k)
    rows = np.concatenate([i, k + i, 2 * k + i, 3 * k + i])
    cols = np.concatenate([k + i, 2 * k + i, 3 * k + i, np.full(k, 4 * k)])
    return cc_ref.csr(rows, cols, 4 * k + 1)


def hub_winner(leaves, seed):
    """the leaf that the hub of star_hub_last(leaves) is matched with under RANDOM"""
    i = np.arange(leaves)
    key = edge_keys(i, np.full(leaves, leaves), "random", seed, None)
    return int(np.lexsort((i, key))[0])


# the small named graphs: colouring's, which the ABI test checks on the host and the GPU test against the model
SMALL = color_ref.SMALL
GRAPHS = dict(color_ref.GRAPHS)
# rows of W - 1, W and W + 1 entries for W = 4, 16, 64 lanes
GROUP_GRAPHS = {
    "cliques4_6": lambda: kcore_ref.cliques([4, 5, 6]),
    "cliques16_18": lambda: kcore_ref.cliques([16, 17, 18]),
    "cliques64_66": lambda: kcore_ref.cliques([64, 65, 66]),
}
HUB_GRAPHS = {
    "star_chunk_minus_1": lambda: star_hub_last(CHUNK - 1),
    "star_chunk": lambda: star_hub_last(CHUNK),
    "star_chunk_plus_1": lambda: star_hub_last(CHUNK + 1),
    "star_2chunks_plus_1": lambda: star_hub_last(2 * CHUNK + 1),
    "two_hubs": lambda: two_hubs(CHUNK + 1),
    "hub_live3": lambda: hub_live3(CHUNK + 1),
}
# RANDOM seeds under which the hub of star_2chunks_plus_1 is matched with a leaf of its first, middle and last chunk (the
# last chunk holds ONE entry); found by a search with hub_winner, and the GPU test asserts them from the model again
CHUNK_SEEDS = {0: 4096, 1: 0, 2: 13627}     # chunk number -> seed
