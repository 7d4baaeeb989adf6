"""The certificate dedup (IBFT_FLAG_CERT_DEDUP, csrc/cert_dedup_dev.h) as a Python model, and the inputs its tests share.

The model is a dict keyed by the 117 key bytes (digest32 ‖ sig65 ‖ from20) of the rows without a pre-flag: a key's
representative is its lowest row, the dense batch lists the representatives in ascending order, every row's bit is its
representative's.  `key_hash` / `table_slots` repeat the device's slot hash and slot count, so that the model can lay out the
table a GPU-test input gets and measure its longest run of occupied slots: shorter than MAX_PROBES, no row can give up
whatever the order of insertion, and the GPU tests may demand exact counts.  Test infrastructure only."""
import random

import numpy as np

from oracle import binding as B
from oracle import wire
from oracle import wire_cert as WC
from oracle import workload as W

import cert_cases as CC
import cert_verdict_cases as K

MAX_PROBES = 128          # cdd::MAX_PROBES (tests/test_dev_cert_dedup_host.py compares it with the harness's)
TREE_DEFER_BYTES = 256    # wire::TREE_DEFER_BYTES
M32 = 0xFFFFFFFF


# ---- the model -------------------------------------------------------------------------------------------------
def representatives(keys, pre):
    """keys: one 117-byte key per row; pre: one flag per row → (rep per row or None, representatives ascending)"""
    first = {}
    for r, (k, p) in enumerate(zip(keys, pre)):
        if not p and k not in first:
            first[k] = r
    rep = [None if p else first[k] for k, p in zip(keys, pre)]
    return rep, sorted(first.values())


def scattered_bits(keys, pre, row_bit):
    rep, _ = representatives(keys, pre)
    return [bool(row_bit[x]) if x is not None else False for x in rep]


def table_slots(rows, cap=0):
    s = 64
    while s < 2 * rows:
        s <<= 1
    if cap:
        c = 1
        while c <= cap // 2:
            c <<= 1
        s = min(s, c)
    return s


def _mix(h, w):
    h = ((h ^ w) * 0x85EBCA6B) & M32
    return ((h << 13) | (h >> 19)) & M32


def key_hash(key):
    """cdd::key_hash: the eight digest words, the sixteen words of r ‖ s, then v"""
    h = 0x9E3779B9
    for i in range(0, 96, 4):
        h = _mix(h, int.from_bytes(key[i:i + 4], "little"))
    h = _mix(h, key[96])
    h ^= h >> 16
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 15)


def longest_run(distinct_keys, slots):
    """the longest run of occupied slots (around the end of the table too) once every key sits in the table by linear
    probing; which slots are occupied does not depend on the order of insertion"""
    taken = [False] * slots
    for k in distinct_keys:
        s = key_hash(k) & (slots - 1)
        while taken[s]:
            s = (s + 1) & (slots - 1)
        taken[s] = True
    if all(taken):
        return slots
    start = taken.index(False)
    best = run = 0
    for i in range(1, slots + 1):
        run = run + 1 if taken[(start + i) % slots] else 0
        best = max(best, run)
    return best


# ---- a tree's keys ---------------------------------------------------------------------------------------------
def tree_keys(tree: WC.Tree):
    """→ (key or None per row — None: the row has a pre-flag in every form —, deferred per row: the rows that get the second
    verdict launch in the two-launch form)"""
    keys, deferred = [], []
    for r in range(tree.n_rows):
        o, nd = tree.rows[r], tree.nodes[r]
        judged = tree.status[r] == WC.OK and tree.digest[r] is not None and len(o.signature) == 65 and len(o.sender) == 20
        keys.append(tree.digest[r] + o.signature + o.sender if judged else None)
        deferred.append(bool(o is not None and ((nd["flags"] & WC.HAS_CERT) or nd["len"] > TREE_DEFER_BYTES)))
    return keys, deferred


def expected_stats(tree: WC.Tree, two_launches: bool):
    """(rows, judged_rows, verdict_rows with the flag on) as ibft_cert_stats reports them when no row gives up"""
    keys, deferred = tree_keys(tree)
    judged = sum(k is not None for k in keys)
    if not two_launches:
        return tree.n_rows, judged, len({k for k in keys if k is not None})
    first = {k for k, d in zip(keys, deferred) if k is not None and not d}
    return tree.n_rows, judged, len(first) + sum(1 for k, d in zip(keys, deferred) if k is not None and d)


def table_is_roomy(tree: WC.Tree):
    """the condition under which the GPU tests demand exact counts: (longest run of occupied slots, MAX_PROBES)"""
    keys, _ = tree_keys(tree)
    return longest_run({k for k in keys if k is not None}, table_slots(tree.n_rows)), MAX_PROBES


# ---- the inputs of tests/test_gpu_cert_dedup.py (built once per process) -------------------------------------------
H, RND = 5, 2
COUNT_SEEDS = {7: 921, 40: 922}   # seeds of the rounds; tests/test_dev_cert_dedup_host.py fails if a table is not roomy
EDGE_SEED, EDGE_VALIDATORS = 923, 48
EDGE_JUDGED = (1, 63, 64, 65, 129)
_cache = {}


def count_inputs(n):
    """(round, {label: messages}): honest_round_change_set of n validators as root ROUND_CHANGE messages, and inside a root
    PREPREPARE's RoundChangeCertificate"""
    if ("count", n) not in _cache:
        r = W.make_round(n, COUNT_SEEDS[n], height=H, round_=1)
        rcs = CC.honest_round_change_set(r, H, RND)
        _cache[("count", n)] = (r, {"roots": [m.encode() for m in rcs], "nested": [CC.preprepare_with_rcc(r, H, RND, rcs).encode()]})
    return _cache[("count", n)]


def edge_round():
    if "edge_round" not in _cache:
        _cache["edge_round"] = W.make_round(EDGE_VALIDATORS, EDGE_SEED, height=H, round_=1)
    return _cache["edge_round"]


def edge_inputs():
    """{judged rows: messages}: root ROUND_CHANGE messages of distinct carriers whose certificates (cert_verdict_cases.
    sized_certificate) hold the SAME proposal message and PREPAREs — 1 row; 3 × 21; 2 × 32; 5 × 13 (the last certificate's
    last PREPARE is row 64); 3 × 43 (the second and third copy of every nested message lie in the words after its first)"""
    if "edge" not in _cache:
        r = edge_round()
        out = {1: [CC.round_change(r, 0, H, RND).encode()]}
        for judged, (carriers, children) in {63: (3, 20), 64: (2, 31), 65: (5, 12), 129: (3, 42)}.items():
            out[judged] = [K.sized_certificate(r, H, 1, c, children).encode() for c in range(carriers)]
            assert carriers * (1 + children) == judged
        _cache["edge"] = out
    return _cache["edge"]


def flipped_inputs():
    """three ROUND_CHANGE messages whose certificates (42 messages each, as the 129-row edge input) nest the same PREPAREs; one of
    them has a flipped signature byte → (messages, the ordinal of that PREPARE among a certificate's children)"""
    if "flipped" not in _cache:
        r = edge_round()
        prop = K.proposer(r.n, H, 1)
        hsh = B.proposal_hash(r.raw, 1)
        pp = CC.preprepare(r, prop, H, 1)
        prs = [CC.prepare(r, i, H, 1, h=hsh) for i in [i for i in range(r.n) if i != prop][:41]]
        bad = 40          # the last one: rows 3 + 41, 45 + 41 and 87 + 41 of the tree, one in each of its three verdict words
        sig = bytearray(prs[bad].signature)
        sig[40] ^= 0x10
        prs[bad].signature = bytes(sig)
        pcb = wire.prepared_certificate(pp, prs)
        msgs = [CC.round_change(r, c, H, RND, wire.Proposal(r.raw, 1), pcb).encode() for c in range(3)]
        _cache["flipped"] = (msgs, 1 + bad)
    return _cache["flipped"]


def gpu_input_trees():
    """(label, tree) of every input the GPU tests demand exact counts for"""
    out = []
    for n in COUNT_SEEDS:
        r, d = count_inputs(n)
        out += [(f"count n={n} {label}", WC.expected_tree(msgs, r.addrs)) for label, msgs in d.items()]
    r = edge_round()
    out += [(f"edge {j}", WC.expected_tree(msgs, r.addrs)) for j, msgs in edge_inputs().items()]
    out.append(("flipped", WC.expected_tree(flipped_inputs()[0], r.addrs)))
    return out


# ---- key sets for the CPU harness ------------------------------------------------------------------------------
def random_key(rng):
    return bytes(rng.randrange(256) for _ in range(117))


def key_set(kind, n, seed=5):
    """→ (keys[n], pre[n], row_bit[n]): row_bit is what a row gets when judged on its own — a function of the key, 0 for a
    pre-flagged row"""
    rng = random.Random(seed * 1000 + n)
    base = random_key(rng)
    pre = [0] * n
    if kind == "all_same":
        keys = [base] * n
    elif kind == "all_distinct":
        keys = [random_key(rng) for _ in range(n)]
    elif kind == "v_only":            # equal in digest, r, s and From: the last signature byte alone
        keys = [base[:96] + bytes([i % 4]) + base[97:] for i in range(n)]
    elif kind == "digest_byte":       # equal in signature and From: one digest byte
        keys = [base[:(i % 32)] + bytes([base[i % 32] ^ (1 + i % 3)]) + base[(i % 32) + 1:] for i in range(n)]
    elif kind == "from_byte":         # equal in digest and signature: one From byte (no real message can be built like this)
        keys = [base[:97 + i % 20] + bytes([base[97 + i % 20] ^ (1 + i % 2)]) + base[98 + i % 20:] for i in range(n)]
    elif kind == "duplicates":        # a few keys, many copies, in shuffled positions
        pool = [random_key(rng) for _ in range(max(1, n // 9))]
        keys = [rng.choice(pool) for _ in range(n)]
    elif kind == "pre_among_duplicates":
        pool = [random_key(rng) for _ in range(max(1, n // 9))]
        keys = [rng.choice(pool) for _ in range(n)]
        pre = [1 if i % 3 == 0 else 0 for i in range(n)]   # row 0, the lowest copy of its key, among them
        pre[-1] = 2
    else:
        raise ValueError(kind)
    verdict = {}
    for k in keys:
        verdict.setdefault(k, len(verdict) % 3 != 1)       # every third key is a bad signature: all its copies must read 0
    row_bit = [0 if p else int(verdict[k]) for k, p in zip(keys, pre)]
    return keys, pre, row_bit


KEY_SET_KINDS = ["all_same", "all_distinct", "v_only", "digest_byte", "from_byte", "duplicates", "pre_among_duplicates"]
KEY_SET_SIZES = [1, 2, 63, 64, 65, 1000]


def columns(keys, pre):
    """the verdict columns of n rows with room for the dense batch behind them"""
    n = len(keys)
    d, s, f, p = (np.zeros((2 * n, w), dtype=np.uint8) for w in (32, 65, 20, 1))
    for r, k in enumerate(keys):
        d[r], s[r], f[r] = np.frombuffer(k[:32], np.uint8), np.frombuffer(k[32:97], np.uint8), np.frombuffer(k[97:], np.uint8)
    p[:n, 0] = pre
    return d, s, f, p
