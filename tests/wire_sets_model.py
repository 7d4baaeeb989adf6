"""A plain model of the wire route under a family of validator sets (ibft_set_height_sets, ibft_verify_senders_wire_sets):
dictionaries and Python integers, no tables and no device code.

  a set        an ordered list of (address, power) in which a repeated address keeps its FIRST position and its LAST power
               (ibft_set_validators); the index of an address is its position among the distinct addresses
  the map      n_ranges + 1 strictly increasing heights and n_ranges set indices: heights in [first[k], first[k+1]) are
               judged under set range_set[k], every other height under none (−1)
  a row        (status, has_view, height) of the parsed message → its set; a sender and the verdict of the signature check
               against the UNION of the family → the verdict under the row's set and the sender's index there
  a tally      per set, over its rows in batch order: ValidatorManager.HasQuorum (core/validator_manager.go:77-96, 128-136)
"""
E_OK, E_INVAL, E_NOVALSET, E_TOOBIG = 0, -1, -5, -7
RANGES_MAX = 4096   # IBFT_HEIGHT_RANGES_MAX
WIRE_OK = 0


def check_height_sets(have_ctx, n_ranges, first, range_set, n_sets):
    """what ibft_set_height_sets answers, its checks in the documented order; n_sets: None without a family → (code, clears)"""
    if not have_ctx:
        return E_INVAL, False
    if n_ranges == 0:
        return E_OK, True
    if first is None or range_set is None or any(first[k + 1] <= first[k] for k in range(n_ranges)):
        return E_INVAL, False
    if n_ranges > RANGES_MAX:
        return E_TOOBIG, False
    if n_sets is None:
        return E_NOVALSET, False
    if any(s >= n_sets for s in range_set[:n_ranges]):
        return E_INVAL, False
    return E_OK, False


def set_of_height(first, range_set, h):
    for k in range(len(range_set)):
        if first[k] <= h < first[k + 1]:
            return range_set[k]
    return -1


def row_set(status, has_view, height, first, range_set):
    if status != WIRE_OK or not has_view:
        return -1
    return set_of_height(first, range_set, height)


class Set:
    def __init__(self, members):
        self.order, self.power = [], {}
        for a, p in members:
            if a not in self.power:
                self.order.append(a)
            self.power[a] = int(p)
        self.index = {a: i for i, a in enumerate(self.order)}
        self.quorum = 2 * sum(self.power.values()) // 3 + 1


def judge(sets, rows):
    """sets: [Set]; rows: [(set or −1, sender bytes, union verdict)] in batch order → (bits, vidx, per-set dicts)"""
    bits, vidx = [], []
    seen = [set() for _ in sets]
    valid = [0] * len(sets)
    for s, sender, ok in rows:
        i = sets[s].index.get(sender, -1) if (s >= 0 and ok) else -1
        bits.append(i >= 0)
        vidx.append(i)
        if i >= 0:
            valid[s] += 1
            seen[s].add(sender)
    tallies = []
    for k, st in enumerate(sets):
        power = sum(st.power[a] for a in seen[k])
        tallies.append(dict(power=power, quorum=st.quorum, valid_rows=valid[k], distinct_senders=len(seen[k]),
                            has_quorum=int(power >= st.quorum)))
    return bits, vidx, tallies
