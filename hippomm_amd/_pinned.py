"""Pinned host staging for host-to-device copies: the buffer, and the event behind the last copy issued from it.

The discipline is the same wherever a pinned buffer is reused: wait() before the host writes it again, mark() right after the
copy (before the kernels that follow on that stream, so a later wait() does not wait for them), and stage() to replace a
buffer that is too small.  Nothing here takes a lock: a table belongs to whoever holds its caller's lock."""
from __future__ import annotations

import torch


class PinnedStage:
    """A pinned tensor of `shape` (`capacity` = its first dimension), `host` its numpy view, `last_upload` the event behind
    the last host-to-device copy issued from it (None: none yet)."""

    def __init__(self, shape, dtype=torch.uint8):
        self.pinned = torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
        self.host = self.pinned.numpy()
        self.capacity = self.pinned.shape[0]
        self.last_upload = None

    def wait(self) -> None:
        """Until the last copy issued from the buffer has left it."""
        if self.last_upload is not None:
            self.last_upload.synchronize()

    def mark(self, stream=None):
        """Right after a copy from the buffer on `stream` (None: the current one) -> the event behind it."""
        self.last_upload = torch.cuda.Event()
        self.last_upload.record(stream)
        return self.last_upload


def stage(table: dict, key, shape, dtype=torch.uint8, keep: int = None) -> PinnedStage:
    """table[key] when it is at least `shape` in every dimension; else a new PinnedStage of `shape` under `key`, once the
    entry it replaces has been waited on.  keep: how many entries the table may then hold -- the oldest others are waited on
    and dropped first; None: every other entry stays (a table with one entry per device)."""
    shape = tuple(shape)
    st = table.get(key)
    if st is not None and len(st.pinned.shape) == len(shape) and all(have >= want for have, want in zip(st.pinned.shape, shape)):
        return st
    if st is not None:
        st.wait()
    if keep is not None:
        others = [k for k in table if k != key]
        for k in others[: max(0, len(others) - (keep - 1))]:
            table.pop(k).wait()
    st = table[key] = PinnedStage(shape, dtype)
    return st
