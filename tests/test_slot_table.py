"""SlotTable against a plain list model of CorrBlock's rows: `cat` appends, `x[mask]` keeps in order
(droid_slam/modules/corr.py:52-60).  Host bookkeeping only: no device, no library call."""
import random

import pytest

from droid_backends.pyramid_store import SlotTable


def _check_invariants(table, model, slot_of):
    slots = table.slots
    assert len(table) == len(model) == len(slots)
    assert [slot_of[e] for e in model] == slots          # the edge order is the model's
    assert len(set(slots)) == len(slots)                 # pairwise distinct
    assert all(0 <= s < table.cap for s in slots)
    assert table.free == table.cap - len(slots)


@pytest.mark.parametrize("seed", range(12))
def test_random_sequences_follow_the_list_model(seed):
    rng = random.Random(seed)
    cap = rng.choice([1, 3, 8, 24])
    table, model, slot_of, next_edge = SlotTable(cap), [], {}, 0
    freed_ever, reused = set(), False
    for _ in range(300):
        op = rng.random()
        if op < 0.45:
            n = rng.randint(0, 8)
            live = set(table.slots)
            lowest = [s for s in range(table.cap) if s not in live][:n]
            if n > table.cap - len(model):
                with pytest.raises(RuntimeError, match="grow"):
                    table.alloc(n)
                assert table.slots == [slot_of[e] for e in model]   # a refused alloc changes nothing
                continue
            got = table.alloc(n)
            assert got == lowest                                    # the lowest free slots, ascending
            reused = reused or bool(freed_ever & set(got))
            for s in got:
                slot_of[next_edge] = s
                model.append(next_edge)                             # cat
                next_edge += 1
        elif op < 0.9:
            mask = [rng.random() < 0.7 for _ in model]
            gone = table.keep(mask)
            assert sorted(gone) == sorted(slot_of[e] for e, m in zip(model, mask) if not m)
            freed_ever.update(gone)
            model = [e for e, m in zip(model, mask) if m]           # x[mask]
        else:
            table.grow(table.cap + rng.randint(0, 8))
        _check_invariants(table, model, slot_of)
    assert reused, "the sequence never reused a freed slot: it does not exercise the free set"


def test_alloc_is_lowest_first_and_freed_slots_come_back():
    t = SlotTable(6)
    assert t.alloc(4) == [0, 1, 2, 3]
    assert t.keep([True, False, True, False]) == [1, 3]
    assert t.slots == [0, 2]
    assert t.alloc(3) == [1, 3, 4]
    assert t.slots == [0, 2, 1, 3, 4]
    assert t.alloc(0) == []


def test_alloc_beyond_the_capacity_raises_until_grown():
    t = SlotTable(2)
    t.alloc(2)
    with pytest.raises(RuntimeError, match="grow"):
        t.alloc(1)
    t.grow(4)
    assert t.alloc(2) == [2, 3] and t.cap == 4
    with pytest.raises(ValueError):
        t.grow(3)


def test_bad_arguments():
    with pytest.raises(ValueError):
        SlotTable(0)
    t = SlotTable(3)
    t.alloc(2)
    with pytest.raises(ValueError, match="mask"):
        t.keep([True])
    with pytest.raises(ValueError):
        t.alloc(-1)


def test_slots_is_a_copy():
    t = SlotTable(3)
    t.alloc(2)
    t.slots.append(7)
    assert t.slots == [0, 1]
