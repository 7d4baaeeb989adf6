"""The per-device key cache (key_cache_map / key_cache_unmap / recount_built in csrc/ibftgpu.hip) where a mistake is a false
accept: validators the budget leaves without a slot, a pool that grows while other contexts hold built tables in it, and a
recycled slot whose old key and table still lie in device memory.

The pool belongs to the process, so in a suite run its capacity and free list are whatever the earlier tests left.  Every
scenario here therefore runs in a FRESH child process (tests/key_cache_child.py), one at a time; the child makes its inputs,
takes its expectations from the CPU oracle and from tests/key_cache_model.py, and prints a marker when all held.  The CPU
tests below run the children's input functions — the model's predictions for each call sequence and the conditions the
inputs must meet — without a GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "key_cache_child.py")


def run_child(scenario, *args, env=None, timeout=240):
    e = dict(os.environ, **(env or {}))
    p = subprocess.run([sys.executable, CHILD, ROOT, scenario, *map(str, args)], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=timeout)
    marker = f"KEY_CACHE_{scenario.upper()}_OK"
    assert p.returncode == 0 and marker in p.stdout, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"


@pytest.mark.gpu
@pytest.mark.parametrize("warm_lanes,cold_lanes", [(1, 1), (8, 16), (64, 128)])
def test_validators_beyond_the_budget_stay_on_the_recover_path(warm_lanes, cold_lanes):
    """IBFT_QTAB_BUDGET_GB=1: 1 638 slots for 1 700 validators.  The 62 without a slot are decided by the cold kernel behind
    every warm kernel form (lane, group, wave: the `sl < 0` branches), in seals, senders and recover mode, with every kind of
    bad row on both sides; the all-warm exit is never taken; a set that fits afterwards is all-warm after one more pass."""
    run_child("overflow", warm_lanes, cold_lanes, timeout=420,
              env={"IBFT_QTAB_BUDGET_GB": "1", "IBFT_WARM_LANES": str(warm_lanes), "IBFT_COLD_LANES": str(cold_lanes)})


@pytest.mark.gpu
def test_a_budget_of_zero_turns_the_cache_off():
    run_child("budget0", env={"IBFT_QTAB_BUDGET_GB": "0"})


@pytest.mark.gpu
def test_tables_survive_the_growth_of_the_pool():
    """A's 64 built tables move to new buffers when B (200 validators, 32 of them A's), then C (600) make the pool grow: A is
    all-warm with oracle verdicts right after each move, B counts A's 32 tables at once, closing gives the slots back."""
    run_child("growth")


@pytest.mark.gpu
def test_a_recycled_slot_forgets_its_owner_across_contexts():
    """A leaves X (B still holds it), B closes, A takes Z: Z sits in slots whose old keys and tables are still in memory.  No
    seal of a past owner claimed by any Z validator is accepted — before, while and after Z's own tables are built."""
    run_child("recycle")


@pytest.mark.gpu
def test_a_recycled_slot_forgets_its_owner_within_one_context():
    """10 of 64 validators replaced: with 54 tables the warm kernel runs, and the 10 × 10 rows "a leaver's seal claimed by a
    newcomer" are all turned down although each newcomer's slot still holds a leaver's complete table."""
    run_child("rotation")


@pytest.mark.parametrize("scenario", ["overflow", "budget0", "growth", "recycle", "rotation"])
def test_scenario_inputs_and_model_predictions(scenario):
    """no GPU: what each child checks before it opens a context — every kind of bad row on each side of the budget's edge, the
    disjoint sets, the oracle turning down exactly the spoiled rows, the model's slots and tables for the call sequence"""
    import key_cache_child as K
    K.INPUTS[scenario]()


def test_model_counts_referrers_and_budget():
    from key_cache_model import SLOT_BYTES, KeyCacheModel
    a = [bytes([i]) * 20 for i in range(8)]
    m = KeyCacheModel(5 * SLOT_BYTES + 7)
    assert m.set_validators("p", a[:4] + a[:2]) == ([], 0) and m.slots_in_use == 4          # repeated addresses: one slot
    m.learned(a[:3])
    assert m.set_validators("q", a[2:8]) == ([3, 4, 5], 1) and m.slots_in_use == 5          # 2, 3 shared, 4 new, 5 … 7 none
    assert m.set_validators("p", a[6:8] + a[2:3]) == ([], 1) and m.slots_in_use == 5        # 0, 1 freed first: 6, 7 fit
    m.close("q")                                                                            # 3, 4 go; 2 stays through p
    assert m.slots_in_use == 3 and m.tables("p") == 1
    assert m.set_validators("q", a[:1]) == ([], 0)                                          # a freed slot remembers nothing
    m.close("p"), m.close("q")
    assert m.slots_in_use == 0 and not m.built
