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


# ---- the same in numpy: key columns of up to 262 145 rows for tests/test_gpu_cert_dedup_kernels.py ---------------------
# Keys are (n, 117) uint8 arrays here.  tests/test_dev_cert_dedup_host.py holds np_key_hash and np_longest_run to key_hash
# and longest_run above, and checks that the table of every input the GPU test demands exact results for is roomy.
NP_NO_REP = 0xFFFFFFFF


def np_key_hash(keys):
    """key_hash of every row → uint32[n]"""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    w = np.ascontiguousarray(keys[:, :96]).view("<u4").astype(np.uint64)

    def mix(h, x):
        h = ((h ^ x) * np.uint64(0x85EBCA6B)) & np.uint64(M32)
        return ((h << np.uint64(13)) | (h >> np.uint64(19))) & np.uint64(M32)
    h = np.full(len(keys), 0x9E3779B9, dtype=np.uint64)
    for i in range(24):
        h = mix(h, w[:, i])
    h = mix(h, keys[:, 96].astype(np.uint64))
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return (h ^ (h >> np.uint64(15))).astype(np.uint32)


def np_distinct(keys):
    """→ (the distinct rows of keys, every row's index among them)"""
    v = np.ascontiguousarray(keys, dtype=np.uint8).view(np.dtype((np.void, keys.shape[1])))[:, 0]
    u, inv = np.unique(v, return_inverse=True)
    return u.view(np.uint8).reshape(len(u), keys.shape[1]), inv.reshape(-1)


def np_longest_run(distinct_keys, slots):
    """longest_run for an array of distinct keys"""
    if len(distinct_keys) == 0:
        return 0
    if len(distinct_keys) >= slots:
        return slots
    home = np.sort((np.uint64(slots - 1) & np.asarray(np_key_hash(distinct_keys), dtype=np.uint64)).astype(np.int64))
    # linear probing on an unbounded line: the i-th key in order of its home slot sits at max_{j ≤ i}(home_j + i − j); keys
    # pushed past the end come in again from slot 0 and push what sits there, which may push more past the end: repeat with
    # that many keys in front until the number is stable (fewer keys than slots leave a free slot that cuts every run)
    over = 0
    while True:
        home2 = np.concatenate([np.zeros(over, np.int64), home])      # the wrapped keys probe from slot 0 on
        i = np.arange(len(home2), dtype=np.int64)
        pos = i + np.maximum.accumulate(home2 - i)
        now_over = int((pos >= slots).sum())
        if now_over == over:
            break
        over = now_over
    pos = pos[pos < slots]                                             # those that fall off the end are the ones in front
    taken = np.zeros(slots, dtype=bool)
    taken[pos] = True
    free = np.nonzero(~taken)[0]
    return int((np.diff(np.concatenate([free, [free[0] + slots]])) - 1).max())


def np_reference(keys, pre):
    """→ (rep per row, NP_NO_REP for a pre-flagged one; the dense batch's source rows, ascending; every row's verdict bit when a
    dense row's bit is: no pre-flag and the low bit of digest byte 0)"""
    n = len(keys)
    judged = np.asarray(pre) == 0
    _, inv = np_distinct(keys)
    first = np.full(int(inv.max()) + 1, n, dtype=np.int64)
    np.minimum.at(first, inv[judged], np.nonzero(judged)[0])
    rep = np.where(judged, first[inv], NP_NO_REP).astype(np.int64)
    dense_rows = np.nonzero(judged & (rep == np.arange(n)))[0]
    rep_bit = (keys[np.where(judged, rep, 0), 0] & 1).astype(bool)
    return rep, dense_rows, judged & rep_bit


KERNEL_SIZES = {"words": [1, 63, 64, 65], "workgroup": [255, 256, 257], "tiles": [1023, 1024, 1025, 2049],
                "count": [16383, 16384, 16385],      # 64 count workgroups exactly, then the second pass of its loop
                "65 tiles": [65537], "257 tiles": [262145]}
KERNEL_KINDS = ["one_key", "one_key_bit0", "mod16", "mirror", "all_distinct", "v_only", "from_byte", "digest_byte", "pre_lowest", "pre_wavefront",
                "pre_all"]
KERNEL_SEED = 31      # tests/test_dev_cert_dedup_host.py fails if a table is not roomy: change it then


def kernel_input(kind, n, seed=KERNEL_SEED):
    """→ (keys (n, 117) uint8, pre uint8[n]) of tests/test_gpu_cert_dedup_kernels.py, built without row loops"""
    rng = np.random.default_rng([seed, n, KERNEL_KINDS.index(kind)])
    r = np.arange(n)
    pre = np.zeros(n, dtype=np.uint8)
    base = rng.integers(0, 256, 117, dtype=np.uint8)

    def pool(count):
        p = rng.integers(0, 256, (count, 117), dtype=np.uint8)
        p[:, 0] = (p[:, 0] & 0xFE) | (np.arange(count) & 1)            # every second key's bit is 0: all its copies must read 0
        return p
    if kind in ("one_key", "one_key_bit0"):                             # n lanes contend on one word; the representative is row 0
        base[0] = (base[0] & 0xFE) | (kind == "one_key")
        keys = np.tile(base, (n, 1))
    elif kind in ("mod16", "pre_lowest"):                               # every wavefront touches every slot
        keys = pool(16)[r % 16]
        if kind == "pre_lowest":
            pre[:16] = 1 + (r[:16] % 3)                                 # the lowest row of every key: the next one up represents it
    elif kind in ("mirror", "pre_wavefront"):                           # rows r and n − 1 − r: the upper half's representative lies tiles away
        keys = pool((n + 1) // 2)[np.minimum(r, n - 1 - r)]
        if kind == "pre_wavefront":
            pre[64:128] = 2                                             # (a whole wavefront where there is a second one …
            if n <= 64:
                pre[:] = 2                                              # … else the only one)
    elif kind == "all_distinct":
        keys = pool(n)
    elif kind == "pre_all":                                             # dense = 0: nothing gathered, all bits 0
        keys = pool(16)[r % 16]
        pre[:] = 1 + (r % 3)
    elif kind == "v_only":                                              # equal in digest, r, s and From
        keys = np.tile(base, (n, 1))
        keys[:, 96] = r % 4
    elif kind == "from_byte":                                           # equal in digest and signature: the hash does not tell them apart
        keys = np.tile(base, (n, 1))
        keys[r, 97 + r % 20] ^= (1 + r % 2).astype(np.uint8)
    elif kind == "digest_byte":
        keys = np.tile(base, (n, 1))
        keys[r, r % 32] ^= (1 + r % 3).astype(np.uint8)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(keys), pre


def kernel_input_run(keys, pre, cap=0):
    """(longest run of occupied slots in the table the input gets, MAX_PROBES)"""
    distinct, _ = np_distinct(keys[np.asarray(pre) == 0]) if (np.asarray(pre) == 0).any() else (keys[:0], None)
    return np_longest_run(distinct, table_slots(len(keys), cap)), MAX_PROBES
