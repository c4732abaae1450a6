"""The detector detects: tests/arena.py on CPU tensors.  A byte planted in a guard (inside the arena's own allocation) must fail
``check_guards`` with the right buffer, side and offset; an untouched arena must pass.  This is what lets a guard failure of
tests/test_gpu_memory_contract.py be believed, and a pass too."""
import pytest
import torch

import arena as A


def _arena(pattern="ones"):
    ar = A.GuardedArena(A.needed_bytes([1000, 4096, 37, 0]), "cpu", A.PATTERNS[pattern])
    views = [ar.carve(1000, "inputs"), ar.carve(4096, "workspace", align=16), ar.carve(37, "out"), ar.carve(0, "empty")]
    return ar, views


@pytest.mark.parametrize("pattern", list(A.PATTERNS))
def test_untouched_arena_passes_and_views_are_poisoned(pattern):
    ar, views = _arena(pattern)
    ar.check_guards()
    byte = A.PATTERNS[pattern] & 0xFF
    for v, size in zip(views, (1000, 4096, 37, 0)):
        assert v.numel() == size and v.dtype == torch.uint8
        assert bool((v == byte).all()) and ar.high_water(v) == -1 and ar.is_pattern(v)
    # writes INSIDE the carved views are the call's own business
    for v in views:
        v.fill_(0x5A)
    ar.check_guards()


def test_alignment_of_carves():
    ar, (a, ws, out, _) = _arena()
    assert a.data_ptr() % 256 == 0 and out.data_ptr() % 256 == 0
    assert ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 != 0            # base + 16: the weakest alignment the header accepts
    assert (ws.data_ptr() - 16) % 256 == 0
    c = ar.carves
    for prev, nxt in zip(c, c[1:]):                                        # a full guard on each side of every buffer
        assert nxt.start - prev.end >= 2 * A.GUARD_BYTES
    assert c[0].start >= A.GUARD_BYTES
    with pytest.raises(ValueError):
        A.GuardedArena(1 << 20, "cpu", guard=1024)                         # the guard width is a condition


@pytest.mark.parametrize("name,index", [("inputs", 0), ("workspace", 1), ("out", 2), ("empty", 3)])
@pytest.mark.parametrize("side,distance", [("before", 1), ("before", A.GUARD_BYTES), ("after", 0), ("after", A.GUARD_BYTES - 1),
                                           ("after", 300)])
def test_planted_guard_byte_is_found_and_named(name, index, side, distance):
    ar, views = _arena()
    c = ar.carves[index]
    at = c.start - distance if side == "before" else c.end + distance      # inside the arena's own allocation
    ar.bytes[at] = 0x12
    with pytest.raises(A.GuardViolation) as exc:
        ar.check_guards()
    e = exc.value
    assert (e.name, e.side, e.offset, e.found, e.expected) == (name, side, at - c.start, 0x12, 0xFF)
    assert name in str(e) and side in str(e) and str(at - c.start) in str(e)
    assert not ar.guards_intact()
    ar.bytes[at] = 0xFF
    ar.check_guards()


def test_first_offending_offset_is_the_lowest_address():
    ar, views = _arena("zeros")
    c = ar.carves[1]
    for d in (700, 9, 4000):
        ar.bytes[c.end + d] = 1
    with pytest.raises(A.GuardViolation) as exc:
        ar.check_guards()
    assert (exc.value.name, exc.value.side, exc.value.offset) == ("workspace", "after", c.end - c.start + 9)


def test_a_pattern_is_four_bytes_wide():
    ar = A.GuardedArena(A.needed_bytes([10, 10]), "cpu", 0x11223344)
    v = ar.carve(10, "odd")                                                # 10 bytes: the guard behind starts mid-pattern
    w = ar.carve(10, "next", align=16)
    ar.check_guards()
    assert v.tolist() == [0x44, 0x33, 0x22, 0x11, 0x44, 0x33, 0x22, 0x11, 0x44, 0x33]
    ar.bytes[ar.carves[0].end] = 0x33                                      # the right byte of the pattern at the wrong phase
    with pytest.raises(A.GuardViolation) as exc:
        ar.check_guards()
    assert (exc.value.offset, exc.value.expected) == (10, 0x22)


def test_high_water_and_repoison():
    ar, (a, ws, out, empty) = _arena("big")
    assert ar.high_water(ws) == -1
    ws[100] = 0
    assert ar.high_water(ws) == 100
    ws[4095] = 1
    assert ar.high_water(ws) == 4095
    assert ar.high_water(ws, start=4096) == -1 and not ar.is_pattern(ws, start=100)
    ws[17] = 0x7F                                                          # a write of the pattern's own byte leaves no mark ...
    ar.repoison(ws)
    assert ar.high_water(ws) == -1 and bool((ws == 0x7F).all())
    out.fill_(3)
    assert ar.high_water(out) == 36 and ar.high_water(out, start=37) == -1
    assert ar.high_water(empty) == -1
    ar.check_guards()                                                      # ... and none of this touched a guard
    with pytest.raises(KeyError):
        ar.high_water(ws[4:])                                              # only whole carved views have a place in the arena


def test_put_places_poison_right_behind_an_input():
    ar = A.GuardedArena(A.needed_bytes([12]), "cpu", A.PATTERNS["ones"])
    v = ar.put(torch.arange(3, dtype=torch.float32), "x")
    assert v.numel() == 12 and v.view(torch.float32).tolist() == [0.0, 1.0, 2.0]
    c = ar.carves[0]
    assert ar.bytes[c.end: c.end + 4].tolist() == [0xFF] * 4               # NaN as the fp32 a kernel would read past the end
    ar.check_guards()
    with pytest.raises(MemoryError):
        ar.carve(1 << 20, "too big")
