"""Generate tests/golden/modinv_edges.json: the searched corpus of the safegcd inversions.

Runs the event model (tests/modinv_model.py) over the candidate families of tests/modinv_cases.py, per modulus, and keeps
for every event the first KEEP inputs that show it: single values for the divsteps, the canonical form and the carry-save
form, and quadruples (a value, three partners, its row) for the events that need rows of a wavefront to finish in different
batches.  Also kept: the inputs at the extremes (batches until g = 0, ζ, carry-save limbs).  An optional divsteps event no
candidate reaches is listed under "unreached" with the number of candidates searched.  Seeded and deterministic; no build
is needed.  Run from the repo root:  python tests/golden/make_modinv_edges.py
(--report adds the counts over the whole candidate set and over the random control, for a summary; it writes nothing.)
"""
import collections
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import modinv_cases as MC  # noqa: E402

QUAD_TRIES = 400
RARE = ("close:add3", "close:subM", "cs:out_of_range", "cs:d_called_negative", "cs:d_called_nonnegative")


def search_values(name, m, report=None):
    kept, order = {}, []  # value → {form: events}, insertion order
    hits = {form: collections.Counter() for form in ("divsteps", "canonical", "wave")}
    ext = {}

    def keep(x, a):
        if x not in kept:
            kept[x] = {form: a[form] for form in ("divsteps", "canonical", "wave")}
            order.append(x)

    def extreme(key, val, x, a, better):
        if key not in ext or better(val, ext[key][0]):
            ext[key] = (val, x, a)

    cands = MC.candidates(m)
    for x, fam in cands:
        a = MC.analyse(x, m)
        for form in hits:
            for ev in a[form]:
                if report is not None:
                    report[form][ev] += 1
                if hits[form][ev] < MC.KEEP:
                    hits[form][ev] += 1
                    keep(x, a)
        if x:
            extreme("batches_min", a["batches"], x, a, lambda p, q: p < q)
            extreme("batches_max", a["batches"], x, a, lambda p, q: p > q)
            extreme("zeta_min", a["zeta"][0], x, a, lambda p, q: p < q)
            extreme("zeta_max", a["zeta"][1], x, a, lambda p, q: p > q)
            extreme("limb_min", a["limb"][0], x, a, lambda p, q: p < q)
            extreme("limb_max", a["limb"][1], x, a, lambda p, q: p > q)
    for key, (val, x, a) in ext.items():
        keep(x, a)
    for x in MC.specials(m) + list(MC.NAMED.values()):  # the existing tests' values and the named cases always run
        keep(x % m, MC.analyse(x % m, m))
    unreached = {ev: len(cands) for ev in MC.DIVSTEPS_OPTIONAL if not hits["divsteps"][ev]}
    extremes = {key: [val, "%x" % x] for key, (val, x, a) in sorted(ext.items())}
    return order, kept, extremes, unreached, len(cands)


def search_quads(name, m, order, kept):
    rng = random.Random("modinv quads " + name)
    rare = [x for x in order if set(kept[x]["wave"]) & set(RARE)]
    hits, quads, seen = collections.Counter(), [], set()
    for t in range(QUAD_TRIES):
        if all(hits[ev] >= MC.KEEP for ev in MC.ROWS):
            break
        x, pos = rare[t % len(rare)], t % 4
        xs = rng.sample(order, 3)
        xs.insert(pos, x)
        w = MC.analyse_quad(xs, m)
        evs = sorted(w["events"] | {e for e in w["rows"][pos]["events"] if not e.startswith("ds:")})
        new = [ev for ev in evs if ev in MC.ROWS and hits[ev] < MC.KEEP]
        if new and tuple(xs) not in seen:
            seen.add(tuple(xs))
            for ev in new:
                hits[ev] += 1
            quads.append(dict(values=["%x" % v for v in xs], pos=pos, events=evs, first=w["first"], last=w["last"],
                              batches=w["batches"]))
    return quads


def build(report=None):
    fix = dict(about="searched inputs of the safegcd inversions; made by tests/golden/make_modinv_edges.py", keep=MC.KEEP,
               moduli={})
    for name, m in MC.MODULI.items():
        rep = None if report is None else report.setdefault(name, {f: collections.Counter() for f in MC.FORMS})
        order, kept, extremes, unreached, searched = search_values(name, m, rep)
        quads = search_quads(name, m, order, kept)
        assert len(order) <= MC.MAX_VALUES and len(quads) <= MC.MAX_QUADS
        fix["moduli"][name] = dict(
            searched=searched, values=["%x" % x for x in order],
            events={form: {"%x" % x: kept[x][form] for x in order} for form in ("divsteps", "canonical", "wave")},
            quads=quads, extremes=extremes, unreached=unreached)
    return json.dumps(fix, indent=1, sort_keys=True) + "\n"


def report():
    rep = {}
    text = build(rep)
    fix = json.loads(text)
    for name, m in MC.MODULI.items():
        ctl = {f: collections.Counter() for f in MC.FORMS}
        for x in MC.control(name):
            a = MC.analyse(x, m)
            for form in ("divsteps", "canonical", "wave"):
                ctl[form].update(a[form])
        xs = MC.control(name)
        for i in range(0, len(xs), 4):
            w = MC.analyse_quad(xs[i:i + 4], m)
            ctl["rows"].update(w["events"])
            for r in w["rows"]:
                ctl["rows"].update(e for e in r["events"] if not e.startswith("ds:"))
        cor = {f: collections.Counter() for f in MC.FORMS}
        for form in ("divsteps", "canonical", "wave"):
            for evs in fix["moduli"][name]["events"][form].values():
                cor[form].update(evs)
        for q in fix["moduli"][name]["quads"]:
            cor["rows"].update(q["events"])
        print("modulus %s: %d candidates searched, %d values and %d quadruples kept; extremes %s; unreached %s" % (
            name, fix["moduli"][name]["searched"], len(fix["moduli"][name]["values"]), len(fix["moduli"][name]["quads"]),
            {k: v[0] for k, v in fix["moduli"][name]["extremes"].items()}, fix["moduli"][name]["unreached"]))
        print("  %-10s %-34s %10s %8s %14s" % ("form", "event", "candidates", "corpus", "control(%d)" % MC.CONTROL))
        for form, evs in MC.required().items():
            for ev in evs + (MC.DIVSTEPS_OPTIONAL if form == "divsteps" else []):
                print("  %-10s %-34s %10s %8d %14d" % (form, ev, rep[name][form][ev] if form != "rows" else "-", cor[form][ev],
                                                      ctl[form][ev]))


if __name__ == "__main__":
    if "--report" in sys.argv:
        report()
    else:
        with open(MC.FIXTURE, "w") as f:
            f.write(build())
        print("wrote", MC.FIXTURE)
