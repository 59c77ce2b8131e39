"""Case tables for the MPT subtree digests (csrc/mpt_graph.cuh, csrc/mpt_digest.hip) and the checker's restatement of include/mp2g.h's
rules in plain Python: which proofs are accepted, the occurrences they give their nodes, the reference occurrence, the conflicts (a),
(b), (c), and the sums from the deepest level up, over the tries of tests/mpt_cases.py, the Keccak of tests/keccak_cases.py and the
oracle's curve (tests/ec_cases.py: base_points, negate, orc_sum). No GPU is used here and nothing here calls the code under test.
Every case is the smallest shape at which one part can go wrong; tests/test_mpt_digest_cases.py holds the restatement to what each
case intends.

Leaf (proof) i holds base_points(512)[i % 512] unless the case says otherwise. The builders are cached: every caller gets the same
objects and must leave them unchanged."""
import functools

import numpy as np

import ec_cases as EC
import keccak_cases as K
import mpt_cases as M

NO_NODE = 0xFFFFFFFF
UNREACHED, OK, CONFLICT = range(3)
P = EC.P
SHAPE_OUTPUTS = ("n_leaves", "state", "via", "parent", "entered")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def own_nibbles(info):
    return 1 if info & 3 == M.BRANCH else info >> 8 & 0x7F


def accepted(infos, path, depth, max_depth, status):
    """whether a proof contributes; status None: it counts as OK"""
    if status is not None and status != M.OK:
        return False
    if not 1 <= depth <= max_depth:
        return False
    ptr = 0
    for level in range(depth):
        x = path[level]
        if x >= len(infos):
            return False
        kind = infos[x] & 3
        if (kind != M.LEAF) if level + 1 == depth else (kind not in (M.BRANCH, M.EXTENSION)):
            return False
        ptr += own_nibbles(infos[x])
        if ptr > 64:
            return False
    return ptr == 64


def occurrences(infos, path, depth, key):
    """[(node, parent, level, entered, slot)] of an accepted proof"""
    nib, out, ptr, parent, slot = K.bytes_to_nibbles(key), [], 0, NO_NODE, 0
    for level in range(depth):
        x = path[level]
        out.append((x, parent, level, ptr, slot))
        slot = nib[ptr] if infos[x] & 3 == M.BRANCH else 0
        ptr += own_nibbles(infos[x])
        parent = x
    return out


def shape(infos, paths, depths, keys, status, max_depth):
    """dict of the shape: accepted proofs, ref {node: its reference occurrence}, via, conflict set, child {(parent, slot): node},
    n_rejected"""
    occ = {}
    for i in range(len(depths)):
        path = [int(x) for x in paths[i]]
        if accepted(infos, path, int(depths[i]), max_depth, None if status is None else int(status[i])):
            occ[i] = occurrences(infos, path, int(depths[i]), keys[i])
    via, ref = {}, {}
    for i in sorted(occ):
        for o in occ[i]:
            via.setdefault(o[0], i)
    for x, i in via.items():
        ref[x] = min((o for o in occ[i] if o[0] == x), key=lambda o: o[2])
    conflict, below = set(), {}
    for i in occ:
        for o in occ[i]:
            if o[1:] != ref[o[0]][1:]:  # (a)
                conflict.add(o[0])
                if o[1] != NO_NODE:
                    conflict.add(o[1])
            if o[1] != NO_NODE:
                below.setdefault((o[1], o[4]), set()).add(o[0])
    conflict |= {p for (p, _), xs in below.items() if len(xs) > 1}  # (b)
    grew = True
    while grew:  # (c)
        more = {p for (p, _), xs in below.items() if xs & conflict} - conflict
        conflict |= more
        grew = bool(more)
    return dict(occ=occ, ref=ref, via=via, conflict=conflict, child={ps: min(xs) for ps, xs in below.items()}, n_rejected=len(depths) - len(occ))


def sums(infos, sh, points):
    """{node: (encoding, Weierstrass limbs, leaves)} of every OK node, from the deepest level up"""
    out = {}
    for x in sorted((x for x in sh["ref"] if x not in sh["conflict"]), key=lambda x: -sh["ref"][x][2]):
        kind = infos[x] & 3
        if kind == M.LEAF:
            out[x] = EC.orc_sum(points[sh["via"][x]][None]) + (1,)
            continue
        kids = [sh["child"][(x, s)] for s in range(16 if kind == M.BRANCH else 1) if (x, s) in sh["child"]]
        out[x] = EC.orc_sum(np.stack([out[k][0] for k in kids])) + (sum(out[k][2] for k in kids),)
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """rows: [(proof, key, root)]; a proof is a list of nodes, the root first, or (list, depth) for a depth other than its length.
    A node is its bytes, None (the index n_nodes, which names no node) or (bytes, tag): a further copy of the node under an index of
    its own. by_position: a node is named by (its parent's index, the key's nibble below that parent, its bytes). status: "real"
    (what the walk of tests/mpt_cases.py gives under the roots), None (the call gets NULL) or a list. conflicts: the labels of the
    nodes the case intends to be CONFLICT, as (row, level) of one occurrence each; None for a case that is not about conflicts."""

    def __init__(self, name, rows, points=None, status="real", by_position=False, max_depth=None, conflicts=(), dev_only=False, extra_nodes=()):
        self.name, self.count, self.by_position, self.dev_only, self.intended_conflicts = name, len(rows), by_position, dev_only, conflicts
        proofs = [r[0] if isinstance(r[0], tuple) else (r[0], len(r[0])) for r in rows]
        self.proofs = [[n[0] if isinstance(n, tuple) else n for n in p] for p, _ in proofs]
        self.keys, self.roots = [r[1] for r in rows], [r[2] for r in rows]
        index, self.nodes = {}, []
        rows_idx = []
        for (proof, _), key in zip(proofs, self.keys):
            nib, parent, ptr, slot, idx = K.bytes_to_nibbles(key), None, 0, 0, []
            for node in proof:
                if node is None:
                    idx.append(None)
                    continue
                raw = node[0] if isinstance(node, tuple) else node
                name_ = (parent, slot, node) if by_position else node
                if name_ not in index:
                    index[name_] = len(self.nodes)
                    self.nodes.append(raw)
                idx.append(index[name_])
                parent = index[name_]
                info = M.open_node(raw)
                slot = nib[ptr] if info & 3 == M.BRANCH and ptr < 64 else 0
                ptr += own_nibbles(info) if info & 3 else 0
            rows_idx.append(idx)
        for node in extra_nodes:  # nodes of the table that no listed proof names (never with by_position)
            if node not in index:
                index[node] = len(self.nodes)
                self.nodes.append(node)
        self.max_depth = max_depth or max(1, max((len(p) for p, _ in proofs), default=1))
        self.depths = np.array([d for _, d in proofs], dtype=np.uint32)
        self.paths = np.zeros((self.count, self.max_depth), dtype=np.uint32)
        for i, idx in enumerate(rows_idx):
            self.paths[i, :len(idx)] = [len(self.nodes) if x is None else x for x in idx]
        self.infos = [M.open_node(n) for n in self.nodes]
        self.hashes = [K.keccak256(n) for n in self.nodes]
        base = EC.base_points(512)
        self.points = np.ascontiguousarray(base[np.arange(self.count) % 512] if points is None else points, dtype=np.uint64).reshape(self.count, 5)
        self._status = status

    def key_rows(self):
        return np.frombuffer(b"".join(self.keys), dtype=np.uint8).reshape(self.count, 32)

    def root_rows(self):
        return np.frombuffer(b"".join(self.roots), dtype=np.uint8).reshape(self.count, 32)

    @functools.lru_cache(maxsize=None)
    def real_status(self):
        return np.array([M.walk(self.nodes, self.hashes, self.infos, [int(x) for x in self.paths[i]], int(self.depths[i]), self.keys[i], self.roots[i],
                                M.WORD, self.max_depth)["status"] for i in range(self.count)], dtype=np.uint32)

    def status(self):
        """what the device form is given: an array, or None for NULL"""
        if self._status is None:
            return None
        return self.real_status() if isinstance(self._status, str) else np.array(self._status, dtype=np.uint32)

    @functools.lru_cache(maxsize=None)
    def want(self, host_form=False):
        """(shape dict, {output name: array}) under the statuses the form works with: the host form always walks itself"""
        status = self.real_status() if host_form else self.status()
        sh = shape(self.infos, self.paths, self.depths, self.keys, status, self.max_depth)
        n = len(self.nodes)
        out = {"w": np.zeros((n, 5), dtype=np.uint64), "weierstrass": np.tile(EC.NEUTRAL_WEI, (n, 1)), "n_leaves": np.zeros(n, dtype=np.uint32),
               "state": np.zeros(n, dtype=np.uint32), "via": np.full(n, NO_NODE, dtype=np.uint32), "parent": np.full(n, NO_NODE, dtype=np.uint32),
               "entered": np.full(n, 0xFF, dtype=np.uint8)}
        for x, (_, parent, _, entered, _) in sh["ref"].items():
            out["state"][x], out["via"][x], out["parent"][x], out["entered"][x] = (CONFLICT if x in sh["conflict"] else OK), sh["via"][x], parent, entered
        for x, (w, wei, leaves) in sums(self.infos, sh, self.points).items():
            out["w"][x], out["weierstrass"][x], out["n_leaves"][x] = w, wei, leaves
        levels = 1 + max((o[2] for o in sh["ref"].values()), default=-1)
        out["totals"] = np.array([sh["n_rejected"], len(sh["conflict"]), levels], dtype=np.uint32)
        return sh, out


def trie_rows(trie, keys=None):
    return [(trie.proofs[k], k, trie.root) for k in (trie.keys if keys is None else keys)]


@functools.lru_cache(maxsize=None)
def pair_trie():
    """two leaves under one branch"""
    return M.Trie({M.key_with([3], 40): M.storage_value(M.value32(40)), M.key_with([12], 41): M.storage_value(M.value32(41))})


@functools.lru_cache(maxsize=None)
def wide_trie():
    """300 keys: 1 / 16 / 179 / 201 / 10 nodes on levels 0..4, so two levels cross a 128-lane workgroup and neither is a multiple of it"""
    return M.Trie({K.keccak256(b"mpt wide %d" % i): M.storage_value(M.value32(900 + i)) for i in range(300)})


WIDE_LEVELS = [1, 16, 179, 201, 10]


@functools.lru_cache(maxsize=None)
def twin_trie():
    """two keys that differ in their first nibble alone and store one value: their leaves are the same bytes; and a third key"""
    first = M.key_with([1], 7)
    twin = M.with_nibble(first, 0, 2)
    t = M.Trie({first: M.storage_value(M.value32(1)), twin: M.storage_value(M.value32(1)), M.key_with([5], 9): M.storage_value(M.value32(2))})
    assert t.proofs[first][-1] == t.proofs[twin][-1] and len(t.proofs[first]) == 2
    return t, first, twin


def _mixed_rows():
    """(rows, labels): the damaged paths among the 129 good proofs of the random trie, one after every sixth"""
    good, bad = trie_rows(M.random_trie()), list(M.damaged_path_rows())
    rows, labels = [], []
    for j, r in enumerate(good):
        rows.append(r)
        labels.append("good %d" % j)
        if j % 6 == 5 and bad:
            d = bad.pop(0)
            rows.append((d[1], d[2], d[3]))
            labels.append(d[0])
    assert not bad
    return rows, labels


# what the shape alone can and cannot refuse of the damaged paths, when no status tells it
MIXED_REJECTED_WITHOUT_STATUS = ("a path cut one short", "the leaf repeated", "an index equal to n_nodes", "depth 0", "a leaf of 62 nibbles at the root",
                                 "an extension of 63 nibbles after 2", "a branch after 64 nibbles", "an embedded child on the way, key 0",
                                 "an embedded child on the way, key 1")
MIXED_ACCEPTED_WITHOUT_STATUS = ("a sound proof", "a wrong root", "the key's first nibble flipped under a full branch", "a 33-byte value")


@functools.lru_cache(maxsize=None)
def cases():
    base = EC.base_points(512)
    p = base[0]
    pair, rnd = pair_trie(), M.random_trie()
    single = M.Trie({M.key_with([], 30): M.storage_value(M.value32(30))})
    ext = M.extension_tries()
    out = [
        Case("one proof of depth 1", trie_rows(single)),
        Case("P and -P under one branch", trie_rows(pair), points=np.stack([p, EC.negate(p)])),
        Case("P and P under one branch", trie_rows(pair), points=np.stack([p, p])),
        Case("all leaves neutral", trie_rows(ext[0][1]), points=np.zeros((len(ext[0][1].keys), 5), dtype=np.uint64)),
    ]
    out += [Case("extension trie %d: %s" % (t, name), trie_rows(trie)) for t, (name, trie, _) in enumerate(ext)]
    out += [
        Case("a 65-node path", trie_rows(M.chain_trie())),
        Case("129 random keys", trie_rows(rnd)),
        Case("300 keys, wide levels", trie_rows(wide_trie())),
        Case("every third proof of the random trie", trie_rows(rnd, rnd.keys[::3]), extra_nodes=[n for k in rnd.keys for n in rnd.proofs[k]]),
    ]
    mixed, _ = _mixed_rows()
    out += [Case("damaged paths among good ones, real status", mixed), Case("damaged paths among good ones, no status", mixed, status=None, conflicts=None)]
    # a status that claims OK for what the shape must refuse itself
    small = ext[2][1]
    good = trie_rows(small)
    pr = small.proofs[small.keys[0]]
    depth = len(pr)
    hostile = [([pr[0], None] + pr[2:], small.keys[0], small.root), (pr + [pr[-1]], small.keys[0], small.root), ((pr, 0), small.keys[0], small.root),
               ((pr, depth + 2), small.keys[0], small.root)]
    out.append(Case("a status that claims OK for hostile paths", good + hostile, status=[M.OK] * (len(good) + 4), max_depth=depth + 1, dev_only=True))
    twins, first, twin = twin_trie()
    out += [
        Case("twin leaves, nodes by bytes", trie_rows(twins), conflicts=((0, 1), (0, 0))),
        Case("twin leaves, nodes by position", trie_rows(twins), by_position=True),
    ]
    a, b = pair.keys
    copy = [pair.proofs[a][0], (pair.proofs[a][1], "copy")]
    out += [
        Case("one node under two indices", [(pair.proofs[a], a, pair.root), (copy, a, pair.root), (pair.proofs[b], b, pair.root)], conflicts=((0, 0),)),
        Case("a proof listed twice", trie_rows(pair, [a, b, a])),
        Case("two tries in one table", trie_rows(ext[0][1]) + trie_rows(ext[1][1])),
        Case("no proof", [], extra_nodes=pair.proofs[a]),
    ]
    return tuple(out)


def names():
    return [c.name for c in cases()]


def case(name):
    return cases()[names().index(name)]


def no_node_case():
    """count 2 over an empty node table: arrays only, no Case (no node can be named)"""
    return dict(paths=np.zeros((2, 3), dtype=np.uint32), depths=np.array([1, 3], dtype=np.uint32), keys=np.zeros((2, 32), dtype=np.uint8), totals=[2, 0, 0])


def hostile_info_words(infos):
    """info words that are not the nodes': every kind with all other bits set, the words rotated and reversed"""
    infos = np.array(infos, dtype=np.uint32)
    return [np.roll(infos, 1), infos[::-1].copy()] + [np.full(len(infos), 0xFFFFFFFC | k, dtype=np.uint32) for k in (1, 2, 3)] + \
        [np.full(len(infos), k | n << 8, dtype=np.uint32) for k in (2, 3) for n in (0, 64, 127)]
