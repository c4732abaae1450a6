"""A guarded, poisoned arena: the memory-contract instrument of tests/test_gpu_memory_contract.py.

One uint8 tensor filled with a repeating 4-byte pattern; ``carve`` hands out views of EXACTLY the requested size with a guard
band of pattern bytes on each side.  After a call into the library (and a device synchronisation) ``check_guards`` compares
every guard with the pattern, on the arena's device, and names the buffer, the side and the first offending byte.  The same
pattern is what the call finds in its workspace, in its output buffers and behind the last byte of every input, so a result
that differs between two patterns has read a byte the call does not own or has not written.

Guard width is a condition, not a measurement: max(64 KiB, the largest single row a kernel of the call writes).  The widest row
in this library is 5120 fp32 = 20 KiB (the MLP hidden row of the vision tower is 5120 bf16 = 10 KiB), so 64 KiB covers a kernel
that runs one whole row, or a few, past either end of a buffer.

What the guards CANNOT see: a wild write that lands further than one guard width from the buffer it belongs to (an index
scaled by the wrong stride, a stale pointer).  Such a write hits another carve's bytes, its guards, or memory outside the arena;
only the first two are noticed, and only by luck.  A write of a value equal to the pattern byte is invisible too, which is why the
tests run three patterns.  Reads leave no trace at all: they are caught only as a difference between the outputs under two patterns.

Patterns: 0xFFFFFFFF (NaN as fp32 and bf16, -1 as an int, the MAXIMUM packed top-k key: adversarial for the scan's key buffers),
0x00000000, 0x7F7F7F7F (a huge finite fp32 / bf16, a large positive int).

Plain helper module (device-agnostic: works on CPU tensors, see tests/test_cpu_arena.py); not a fixture plugin.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch

GUARD_BYTES = 64 * 1024
BASE_ALIGN = 256
PATTERNS = {"ones": 0xFFFFFFFF, "zeros": 0x00000000, "big": 0x7F7F7F7F}
_TILE = 1 << 22                      # bytes compared per step of a scan over a large view


class GuardViolation(AssertionError):
    """A guard byte differs from the pattern.  ``offset`` is relative to the first byte of the buffer: negative in the guard
    before it, >= its size in the guard after it; the lowest offending address of the first damaged guard is reported."""

    def __init__(self, name: str, side: str, offset: int, found: int, expected: int):
        self.name, self.side, self.offset, self.found, self.expected = name, side, offset, found, expected
        super().__init__(f"guard {side} buffer '{name}' damaged: first offending byte at offset {offset} from the buffer's start "
                         f"(found 0x{found:02x}, pattern byte 0x{expected:02x})")


class Carve(NamedTuple):
    name: str
    start: int          # arena offsets
    end: int
    before: int         # the guard before is [before, start), the guard after [end, end + guard)


def needed_bytes(sizes, guard: int = GUARD_BYTES) -> int:
    """An arena size that fits carves of `sizes` bytes whatever their alignment."""
    return sum(int(s) + 2 * guard + 2 * BASE_ALIGN for s in sizes) + guard


class GuardedArena:
    def __init__(self, total_bytes: int, device="cpu", pattern: int = PATTERNS["ones"], guard: int = GUARD_BYTES):
        if guard < GUARD_BYTES:
            raise ValueError(f"guard of {guard} bytes is below the {GUARD_BYTES} the contract tests are specified with")
        self.pattern, self.guard = int(pattern) & 0xFFFFFFFF, int(guard)
        self.device = torch.device(device)
        raw = torch.empty(int(total_bytes) + BASE_ALIGN, dtype=torch.uint8, device=self.device)
        skew = (-raw.data_ptr()) % BASE_ALIGN                    # a CPU allocation is not 256-byte aligned by itself
        self._raw = raw
        self.bytes = raw[skew: skew + int(total_bytes)]
        self._pat4 = torch.tensor([(self.pattern >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8, device=self.device)
        self._tile = self._pat4.repeat(_TILE // 4 + 1)           # little-endian, phase-locked to the arena's offset 0
        self._cursor = 0
        self.carves: List[Carve] = []
        self._by_ptr: Dict[int, Carve] = {}
        self._fill(0, self.bytes.numel())

    # ---- pattern ----------------------------------------------------------------------------------------------------------
    def _expected(self, lo: int, hi: int) -> torch.Tensor:
        phase = lo % 4
        return self._tile[phase: phase + (hi - lo)]

    def _fill(self, lo: int, hi: int) -> None:
        for a in range(lo, hi, _TILE):
            b = min(a + _TILE, hi)
            self.bytes[a:b] = self._expected(a, b)

    def _first_diff(self, lo: int, hi: int, last: bool = False) -> Optional[int]:
        """Arena offset of the first (or last) byte of [lo, hi) that differs from the pattern; compared on the device."""
        steps = list(range(lo, hi, _TILE))
        for a in (reversed(steps) if last else steps):
            b = min(a + _TILE, hi)
            bad = self.bytes[a:b] != self._expected(a, b)
            if bool(bad.any()):
                where = torch.nonzero(bad).flatten()
                return a + int(where[-1] if last else where[0])
        return None

    # ---- allocation -------------------------------------------------------------------------------------------------------
    def carve(self, nbytes: int, name: str, align: int = 256) -> torch.Tensor:
        """A view of exactly `nbytes` bytes, a guard on each side.  align=256: what an allocator returns.  A smaller power of two
        (16 is the weakest the header accepts) carves at a 256-byte boundary PLUS `align`: aligned to that and to nothing more."""
        nbytes = int(nbytes)
        if nbytes < 0 or align < 1 or align > BASE_ALIGN or align & (align - 1):
            raise ValueError(f"carve({nbytes}, align={align})")
        before = self._cursor
        start = (before + self.guard + BASE_ALIGN - 1) // BASE_ALIGN * BASE_ALIGN + (align if align < BASE_ALIGN else 0)
        end = start + nbytes
        if end + self.guard > self.bytes.numel():
            raise MemoryError(f"arena of {self.bytes.numel()} bytes cannot fit '{name}' ({nbytes} bytes at {start})")
        c = Carve(name, start, end, before)
        self._cursor = end + self.guard
        self.carves.append(c)
        view = self.bytes[start:end]
        self._by_ptr.setdefault(view.data_ptr(), c)              # (a zero-byte carve shares no address with another: guards lie between)
        return view

    def put(self, data: torch.Tensor, name: str, align: int = 256) -> torch.Tensor:
        """Carve exactly data's bytes and copy them in: an input with poison right behind its last byte."""
        flat = data.contiguous().reshape(-1).view(torch.uint8)
        view = self.carve(flat.numel(), name, align)
        view.copy_(flat)
        return view

    def address(self, view: torch.Tensor) -> int:
        """The address to hand to the library (an empty view has no data_ptr of its own)."""
        return self.bytes.data_ptr() + self._carve_of(view).start

    def _carve_of(self, view: torch.Tensor) -> Carve:
        c = self._by_ptr.get(view.data_ptr())
        if c is None or view.numel() != c.end - c.start:
            raise KeyError("not a view returned by carve()")
        return c

    # ---- checks -----------------------------------------------------------------------------------------------------------
    def check_guards(self) -> None:
        """Call after synchronising the device.  Raises GuardViolation on the first damaged guard."""
        for c in self.carves:
            for side, lo, hi in (("before", c.before, c.start), ("after", c.end, c.end + self.guard)):
                at = self._first_diff(lo, hi)
                if at is not None:
                    raise GuardViolation(c.name, side, at - c.start, int(self.bytes[at]), int(self._pat4[at % 4]))

    def guards_intact(self) -> bool:
        try:
            self.check_guards()
        except GuardViolation:
            return False
        return True

    def repoison(self, view: torch.Tensor) -> None:
        c = self._carve_of(view)
        self._fill(c.start, c.end)

    def high_water(self, view: torch.Tensor, start: int = 0) -> int:
        """Highest offset inside the carved view whose byte differs from the pattern (-1: none does), looking at [start, size)."""
        c = self._carve_of(view)
        at = self._first_diff(c.start + int(start), c.end, last=True)
        return -1 if at is None else at - c.start

    def is_pattern(self, view: torch.Tensor, start: int = 0) -> bool:
        return self.high_water(view, start) < 0
