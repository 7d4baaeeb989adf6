"""A plain model of ibft_verify_senders_wire_views on top of tests/wire_sets_model.py: dictionaries and Python integers, no
tables and no device code.

  the store     messages.Messages: a dict [(type, height, round)][sender] = row, filled with every VALID row in row order — a
                sender's later message of a view replaces the earlier one (messages/messages.go:64).  What is left in it is the
                stored set.
  a key         (height, round, type, proposal hash); keys ordered by their first valid row are the views
  the cap       view v ≥ views_cap: its rows get −2, no record; min(views_cap, n) is what counts
  a record      over S_v — the senders of the stored rows of view v —: ValidatorManager.HasQuorum with the powers of the view's
                set (wire_sets_model.Set), or, for a PREPARE view the proposer table covers, HasPrepareQuorum as
                ibft_tally_prepare documents it: the proposer's seat joins when the proposer is a member, every row of S_v FROM
                the proposer is counted in proposer_rows and any such row voids has_quorum
"""
import wire_sets_model as M

E_OK, E_INVAL, E_NOVALSET, E_TOOBIG = M.E_OK, M.E_INVAL, M.E_NOVALSET, M.E_TOOBIG
PREPARE, COMMIT = 1, 2
VIEW_NONE, VIEW_OVER = -1, -2


def check_call(have_ctx, n, have_off, have_mask, views_cap, offsets_ok, bytes_ok, max_rows, have_family, have_map):
    """what ibft_verify_senders_wire_views answers before it touches the device, its checks in the documented order: the sets
    call's, with views_cap == 0 for a batch that has rows among the argument checks in front"""
    if not have_ctx or (n and (not have_off or not have_mask)):
        return E_INVAL
    if n and views_cap == 0:
        return E_INVAL
    if not offsets_ok or not bytes_ok:
        return E_INVAL
    if n > max_rows:
        return E_TOOBIG
    if not have_family or not have_map:
        return E_NOVALSET
    return E_OK


class Proposers:
    """ibft_set_proposers: addrs[k] proposes round first_round + k of height"""

    def __init__(self, height=0, first_round=0, addrs=()):
        self.height, self.first_round, self.addrs = height, first_round, list(addrs)

    def lookup(self, height, round_):
        if not self.addrs or height != self.height or not self.first_round <= round_ < self.first_round + len(self.addrs):
            return None
        return self.addrs[round_ - self.first_round]


def tally(st, senders, proposer=None):
    """HasQuorum (proposer None) / HasPrepareQuorum over a list of senders under the Set st → the fields of ibft_tally_t"""
    seen = {a for a in senders if a in st.power}
    proposer_rows = 0
    if proposer is not None:
        proposer_rows = sum(1 for a in senders if a == proposer)
        if proposer in st.power:
            seen.add(proposer)
    power = sum(st.power[a] for a in seen)
    return dict(power=power, quorum=st.quorum, valid_rows=len(senders), distinct_senders=len(seen),
                has_quorum=int(power >= st.quorum and proposer_rows == 0), proposer_rows=proposer_rows)


def views(rows, views_cap, sets, proposers=None):
    """rows: [(valid, type, height, round, hash bytes, set, sender bytes)] in batch order →
    (out_view, stored [bool], n_views, records [dict])"""
    proposers = proposers or Proposers()
    n = len(rows)
    store, first, members = {}, {}, {}
    for i, (valid, typ, height, round_, h, s, sender) in enumerate(rows):
        if not valid:
            continue
        store.setdefault((typ, height, round_), {})[sender] = i
        key = (height, round_, typ, bytes(h))
        first.setdefault(key, i)
        members.setdefault(key, []).append(i)
    held = {i for per_view in store.values() for i in per_view.values()}
    stored = [i in held for i in range(n)]
    order = sorted(first, key=first.get)
    cap = min(views_cap, n)
    out_view = [VIEW_NONE] * n
    records = []
    for v, key in enumerate(order):
        for i in members[key]:
            out_view[i] = v if v < cap else VIEW_OVER
        if v >= cap:
            continue
        height, round_, typ, h = key
        s = rows[first[key]][5]
        sv = [rows[i][6] for i in members[key] if stored[i]]
        p = proposers.lookup(height, round_) if typ == PREPARE else None
        rec = dict(height=height, round=round_, type=typ, hash=h, set=s, first_row=first[key], rows=len(members[key]),
                   stored_rows=len(sv), prepare_rule=int(p is not None), senders=sv, proposer=p)
        rec["tally"] = tally(sets[s], sv, p)
        records.append(rec)
    return out_view, stored, len(order), records
