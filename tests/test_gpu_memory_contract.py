"""GPU: the memory contract of the C ABI (include/hippomm_hip.h).  No call may touch or depend on bytes it does not own.

Every entry point that takes a workspace is called through ctypes with EVERY device buffer -- inputs, outputs, workspace,
shadow store, offsets -- carved from a poisoned, guarded arena (tests/arena.py) at its exact documented size.  Per case:

  1. guards intact after the call, under the three poison patterns, with the workspace at 256-byte and at 16-byte alignment;
  2. poison independence: the outputs are bitwise the same under the three patterns (the pattern is in the workspace, the guards,
     the output buffers and right behind the last byte of every input);
  3. correct: bitwise what the Python shim returns for the same inputs (the shims are pinned against the oracles elsewhere);
  4. documented extent: output bytes past what the header says is valid are still pattern;
  5. reuse: case X, then case Y (another shape, another internal path) in the same workspace without re-poisoning: Y's outputs
     equal Y's on a freshly poisoned workspace (stale tickets, flags, tables, counts);
  6. refusal: with workspace_bytes = need - 1 the call returns HMM_E_WORKSPACE and workspace and outputs are still pure pattern.

Every byte these tests write or inspect lies inside the arena's own allocation, and the library is always told a workspace size
that is not larger than the buffer it gets: nothing here provokes a fault.

The cases are data (``CASES``); tools/memory_contract_report.py runs the same cases and writes profiles/memory_contract.json.
"""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu

HMM_E_WORKSPACE = -2
DEV = "cuda"
LAYOUTS = [(p, a) for a in (256, 16) for p in A.PATTERNS]          # (pattern, workspace alignment)


def _L():
    from hippomm_amd import _lib
    _lib.require_gpu()
    return _lib, _lib.load()


def _nbytes(t):
    return t.numel() * t.element_size()


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _u8(t):
    return t.contiguous().reshape(-1).view(torch.uint8).cpu()


class Case:
    """One call: its inputs (device tensors, carved at exactly their size), outputs (name -> bytes), workspace need.

    call(lib, ptr, ws_ptr, ws_bytes) -> status            the ctypes call; ptr: name -> device address
    valid(raw) -> name -> bytes of the output that the header documents as written (default: all of it)
    shim() -> name -> tensor                              what the Python shim returns (compared with the valid bytes)
    """
    entry = family = label = ""
    need = None                      # workspace bytes; None: the call takes no workspace
    refusable = True

    def __init__(self):
        self.inputs, self.outs = {}, {}

    def place_inputs(self, ar):
        return {name: ar.address(ar.put(t, name)) for name, t in self.inputs.items()}

    def valid(self, raw):
        return {name: raw[name].numel() for name in self.outs}

    def compare(self, raw):
        v = self.valid(raw)
        return {name: raw[name][: v[name]] for name in self.outs}

    def shim(self):
        return {}

    def sizes(self):
        return [_nbytes(t) for t in self.inputs.values()] + list(self.outs.values()) + [self.need or 0]

    def __repr__(self):
        return f"{self.entry}[{self.label}]"


class Run:
    """A case laid out in an arena; launch() calls the library."""

    def __init__(self, case, ar, ws_align=256, ws=None):
        self.case, self.ar = case, ar
        self.ptr = case.place_inputs(ar)
        self.out = {name: ar.carve(nb, "out:" + name) for name, nb in case.outs.items()}
        for name, v in self.out.items():
            self.ptr[name] = ar.address(v)
        self.ws = ws if ws is not None else (ar.carve(case.need, "workspace", ws_align) if case.need is not None else None)

    def launch(self, ws_bytes=None):
        _, lib = _L()
        ws_ptr = self.ar.address(self.ws) if self.ws is not None else None
        rc = self.case.call(lib, self.ptr, ws_ptr, self.case.need if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        return rc

    def results(self):
        """Checks the documented extent (4) and returns the comparable bytes of every output."""
        raw = {name: v.cpu().clone() for name, v in self.out.items()}
        for name, nb in self.case.valid(raw).items():
            hw = self.ar.high_water(self.out[name], start=nb)
            assert hw < 0, f"{self.case}: output '{name}' written at byte {hw}, past its documented extent of {nb} bytes"
        return self.case.compare(raw)


def fresh(case, pattern="ones", ws_align=256):
    """The case alone in a fresh arena: (1) guards, (4) extent -> (outputs, high-water offset of the workspace)."""
    ar = A.GuardedArena(A.needed_bytes(case.sizes()), DEV, A.PATTERNS[pattern])
    run = Run(case, ar, ws_align)
    rc = run.launch()
    assert rc == 0, f"{case} under {pattern}/{ws_align}: status {rc}: {_L()[1].hmm_last_error().decode()}"
    ar.check_guards()
    return run.results(), (ar.high_water(run.ws) if run.ws is not None else -1)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for name in a:
        x, y = _u8(a[name]), _u8(b[name])
        assert x.numel() == y.numel(), f"{what}: '{name}' has {x.numel()} bytes against {y.numel()}"
        if not torch.equal(x, y):
            at = int(torch.nonzero(x != y)[0])
            raise AssertionError(f"{what}: output '{name}' differs from byte {at} on ({int((x != y).sum())} of {x.numel()} bytes)")


def check_case(case):
    """Assertions 1-4 (and 6 where the call takes a workspace) for one case."""
    base = None
    for pattern, align in LAYOUTS:
        got, _ = fresh(case, pattern, align)
        if base is None:
            base = got
            want = case.shim()
            torch.cuda.synchronize()
            if want:
                _same({k: got[k] for k in want}, want, f"{case} against its Python shim")
        else:
            _same(base, got, f"{case}: poison {pattern} / workspace alignment {align} against {LAYOUTS[0]}")
    if case.need is not None and case.refusable:
        check_refusal(case)
    return base


def check_refusal(case):
    for pattern in A.PATTERNS:
        ar = A.GuardedArena(A.needed_bytes(case.sizes()), DEV, A.PATTERNS[pattern])
        run = Run(case, ar)
        assert case.need >= 1
        rc = run.launch(case.need - 1)                       # the true size of a workspace one byte short: a status, no launch
        assert rc == HMM_E_WORKSPACE, f"{case}: workspace_bytes = need - 1 = {case.need - 1} gave status {rc}"
        ar.check_guards()
        assert ar.is_pattern(run.ws), f"{case}: refused call wrote its workspace at byte {ar.high_water(run.ws)}"
        for name, v in run.out.items():
            assert ar.is_pattern(v), f"{case}: refused call wrote output '{name}' at byte {ar.high_water(v)}"


def check_reuse(x, y):
    """(5): x then y in ONE workspace (as large as the larger need; each call is told its true size), no re-poisoning between."""
    want, _ = fresh(y, "ones")
    size = max(x.need, y.need)
    for pattern in ("ones", "zeros"):
        ar = A.GuardedArena(A.needed_bytes(x.sizes() + y.sizes() + [size]), DEV, A.PATTERNS[pattern])
        ws = ar.carve(size, "workspace")
        rx, ry = Run(x, ar, ws=ws), Run(y, ar, ws=ws)
        assert rx.launch(size) == 0 and ry.launch(size) == 0
        ar.check_guards()
        rx.results()
        _same(want, ry.results(), f"{y} after {x} in the same workspace ({pattern}) against a fresh workspace")


# =====================================================================================================================
# scan family
# =====================================================================================================================
@functools.lru_cache(maxsize=4)
def _store(n, kind="random"):
    s = _rand((n, 1024), 1000 + n)
    if kind == "zero_rows":                                   # zero-norm rows: NaN similarities, ranked first
        s[[0, n // 2, n - 1]] = 0.0
    if kind == "ties":                                        # 16 distinct rows, each ~n/16 times: the prefilter gives up
        s = s[:16][torch.randint(0, 16, (n,), generator=torch.Generator().manual_seed(3)).to(DEV)].contiguous()
    return s


def _query(seed=7):
    return _rand((1024,), seed)


def _fs(store):
    from hippomm_amd.vector_ops import FeatureStore
    return FeatureStore(store)


class Scan(Case):
    entry = "hmm_cosine_topk"

    def __init__(self, n, k, kind="random"):
        super().__init__()
        _, lib = _L()
        self.n, self.k, self.kind = n, k, kind
        self.family = "scan n<=4096" if n <= 4096 else "scan full sort" if min(k, n) > 1024 else "scan sims buffer" if k > 128 else "scan fused"
        self.label = f"n={n},k={k}" + ("" if kind == "random" else "," + kind)
        self.inputs = {"store": _store(n, kind), "query": _query(n + k)}
        kk = min(k, n)
        self.outs = {"idx": 8 * kk, "sims": 4 * kk, "n_out": 4}          # int64[k'], fp32[k'], int32[1]; k' = min(k, n_rows)
        self.need = lib.hmm_cosine_topk_workspace_bytes(n, k)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk(p["store"], self.n, 1024, p["query"], self.k, p["idx"], p["sims"], p["n_out"], ws, ws_bytes, None)

    def shim(self):
        idx, sims = _fs(self.inputs["store"]).search_device(self.inputs["query"], self.k)
        return {"idx": idx, "sims": sims, "n_out": torch.tensor([min(self.k, self.n)], dtype=torch.int32)}


class ScanKeys(Scan):
    entry = "hmm_cosine_topk_keys"

    def __init__(self, n, k):
        super().__init__(n, k)
        self.outs = {"keys": 8 * k}                                        # [k], 0-padded

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk_keys(p["store"], self.n, 1024, p["query"], self.k, p["keys"], ws, ws_bytes, None)

    def shim(self):
        return {"keys": _fs(self.inputs["store"]).search_keys_device(self.inputs["query"], self.k)}


class Prefilter(Case):
    entry = "hmm_cosine_topk_prefilter"

    def __init__(self, n, k, kind, route):
        super().__init__()
        _, lib = _L()
        self.n, self.k, self.route = n, k, route               # route: "prefilter" | "fallback" | "exact" (below the dispatch limits)
        self.family, self.label = f"prefilter ({route})", f"n={n},k={k},{kind}"
        store = _store(n, kind)
        self.fs = _fs(store).build_shadow()
        assert self.fs._shadow.numel() == lib.hmm_shadow_store_bytes(n)
        self.inputs = {"store": store, "shadow": self.fs._shadow, "query": _query(n + k)}
        kk = min(k, n)
        self.outs = {"idx": 8 * kk, "sims": 4 * kk, "n_out": 4, "stats": 8}
        self.need = lib.hmm_cosine_topk_prefilter_workspace_bytes(n, k)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk_prefilter(p["store"], p["shadow"], self.n, 1024, p["query"], self.k, p["idx"], p["sims"],
                                             p["n_out"], p["stats"], ws, ws_bytes, None)

    def compare(self, raw):
        got = super().compare(raw)
        cand, sat = got["stats"].view(torch.int32).tolist()
        if self.route == "exact":
            assert (cand, sat) == (-1, -1)
        elif self.route == "fallback":                          # the conditional exact scan answered, inside the same call
            assert sat > 0 or cand > 1024, (cand, sat)
        else:
            assert sat == 0 and self.k <= cand <= 1024, (cand, sat)
        return got

    def shim(self):
        stats = torch.empty(2, dtype=torch.int32, device=DEV)
        idx, sims = self.fs.search_prefiltered_device(self.inputs["query"], self.k, stats)
        return {"idx": idx, "sims": sims, "stats": stats}


class ShadowBuild(Case):
    entry, family = "hmm_shadow_store_build", "shadow build"

    def __init__(self, n):
        super().__init__()
        self.n, self.label = n, f"n={n}"
        self.inputs = {"store": _store(n, "zero_rows" if n >= 3 else "random")}
        self.outs = {"shadow": 2048 * n}

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_shadow_store_build(p["store"], self.n, 1024, p["shadow"], 2048 * self.n, None)

    def shim(self):
        return {"shadow": _fs(self.inputs["store"]).build_shadow()._shadow}


class Segmented(Case):
    def __init__(self, lengths, k, prefilter):
        super().__init__()
        _, lib = _L()
        self.k, self.E, self.n, self.prefilter = k, len(lengths), sum(lengths), prefilter
        self.entry = "hmm_cosine_topk_segmented_prefilter" if prefilter else "hmm_cosine_topk_segmented"
        self.family = "segments " + ("small" if self.n <= 1024 * self.E and k <= 64 else "large") + (", k>64" if k > 64 else "")
        self.label = f"E={self.E},n={self.n},k={k},min={min(lengths)}"
        store = _store(self.n)
        self.fs = _fs(store)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=DEV)
        self.inputs = {"store": store, "query": _query(self.n + k), "offsets": offs}
        if prefilter:
            self.inputs["shadow"] = self.fs.build_shadow()._shadow
        self.outs = {"idx": 8 * self.E * k, "sims": 4 * self.E * k, "counts": 4 * self.E}    # -1 / 0 padded: all of it is written
        q = lib.hmm_cosine_topk_segmented_prefilter_workspace_bytes if prefilter else lib.hmm_cosine_topk_segmented_workspace_bytes
        self.need = q(self.n, self.E, k)

    def call(self, lib, p, ws, ws_bytes):
        if self.prefilter:
            return lib.hmm_cosine_topk_segmented_prefilter(p["store"], p["shadow"], self.n, 1024, p["query"], p["offsets"], self.E,
                                                           self.k, p["idx"], p["sims"], p["counts"], ws, ws_bytes, None)
        return lib.hmm_cosine_topk_segmented(p["store"], self.n, 1024, p["query"], p["offsets"], self.E, self.k, p["idx"],
                                             p["sims"], p["counts"], ws, ws_bytes, None)

    def shim(self):
        idx, sims, counts = self.fs.search_segments_device(self.inputs["query"], self.inputs["offsets"], self.k, self.prefilter)
        return {"idx": idx, "sims": sims, "counts": counts}


class Multi(Case):
    entry = "hmm_cosine_topk_multi"

    def __init__(self, n, nq, k):
        super().__init__()
        _, lib = _L()
        self.n, self.nq, self.k, self.kk = n, nq, k, min(k, n)
        self.family = "multi (per-query fallback)" if self.kk > 64 else "multi"
        self.label = f"n={n},q={nq},k={k}"
        self.inputs = {"store": _store(n), "queries": _rand((nq, 1024), 50 + nq)}
        self.outs = {"idx": 8 * nq * k, "sims": 4 * nq * k, "n_out": 4 * nq}
        self.need = lib.hmm_cosine_topk_multi_workspace_bytes(n, nq, k)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk_multi(p["store"], self.n, 1024, p["queries"], self.nq, self.k, p["idx"], p["sims"], p["n_out"],
                                         ws, ws_bytes, None)

    def compare(self, raw):                                      # rows of stride k; the first min(k, n_rows) entries of a row are valid
        return {"idx": raw["idx"].view(torch.int64).view(self.nq, self.k)[:, : self.kk].contiguous(),
                "sims": raw["sims"].view(torch.float32).view(self.nq, self.k)[:, : self.kk].contiguous(), "n_out": raw["n_out"]}

    def shim(self):
        idx, sims = _fs(self.inputs["store"]).search_multi_device(self.inputs["queries"], self.k)
        return {"idx": idx, "sims": sims, "n_out": torch.full((self.nq,), self.kk, dtype=torch.int32)}


class MergeKeys(Case):
    entry, family = "hmm_topk_merge_keys", "merge keys"

    def __init__(self, shard_rows, k):
        super().__init__()
        self.k, self.S, self.label = k, len(shard_rows), f"shards={shard_rows},k={k}"
        q = _query(11)
        self.inputs = {"keys": torch.stack([_fs(_store(r)).search_keys_device(q, k) for r in shard_rows]),
                       "offsets": torch.tensor(np.concatenate([[0], np.cumsum(shard_rows)[:-1]]), dtype=torch.int64, device=DEV)}
        self.outs = {"idx": 8 * k, "sims": 4 * k, "n_out": 4}

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_topk_merge_keys(p["keys"], self.S, self.k, p["offsets"], p["idx"], p["sims"], p["n_out"], None)

    def valid(self, raw):                                        # *n_out entries
        n = int(raw["n_out"].view(torch.int32)[0])
        return {"idx": 8 * n, "sims": 4 * n, "n_out": 4}

    def shim(self):
        from hippomm_amd.vector_ops import merge_keys_device
        idx, sims = merge_keys_device(self.inputs["keys"], self.inputs["offsets"], self.k)
        return {"idx": idx, "sims": sims}


class RankHits(Case):
    entry, family = "hmm_rank_segment_hits", "rank segment hits"

    def __init__(self, lengths, k, keep):
        super().__init__()
        from hippomm_amd.vector_ops import EventStore
        self.k, self.keep, self.E, self.label = k, keep, len(lengths), f"E={len(lengths)},k={k},keep={keep}"
        self.es = EventStore.from_device_rows(_store(sum(lengths)), lengths)
        self.q = _query(13)
        idx, sims, counts = self.es.search_segments_device(self.q, self.es.offsets, k)
        self.inputs = {"idx": idx.clone(), "sims": sims.clone(), "counts": counts.clone()}
        self.outs = {"event": 8 * keep, "row": 8 * keep, "sim": 4 * keep, "n_out": 4}        # -1 / -1 / 0 padded to `keep`

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_rank_segment_hits(p["idx"], p["sims"], p["counts"], self.E, self.k, self.keep, p["event"], p["row"], p["sim"],
                                         p["n_out"], None)

    def compare(self, raw):
        n = int(raw["n_out"].view(torch.int32)[0])
        ev, row, sim = raw["event"].view(torch.int64), raw["row"].view(torch.int64), raw["sim"].view(torch.float32)
        assert ev[n:].eq(-1).all() and row[n:].eq(-1).all() and sim[n:].eq(0).all()
        return {"event": ev[:n].contiguous(), "row": row[:n].contiguous(), "sim": sim[:n].contiguous(), "pad": raw["event"][8 * n:]}

    def shim(self):
        hits = self.es.top_hits(self.q, self.k, self.keep)
        return {"event": torch.tensor([h[0] for h in hits], dtype=torch.int64), "row": torch.tensor([h[1] for h in hits], dtype=torch.int64),
                "sim": torch.tensor([h[2] for h in hits], dtype=torch.float64).float()}


# =====================================================================================================================
# consolidation
# =====================================================================================================================
class Gram(Case):
    entry = "hmm_gram_select"

    def __init__(self, n, kind):
        super().__init__()
        _, lib = _L()
        self.n, self.family, self.label = n, "gram select" + (" (n<=2: no workspace use)" if n <= 2 else ""), f"n={n},{kind}"
        f = _rand((n, 1024), 77 + n)
        if kind == "nothing_kept":                               # every row within 0.9 of row 0: only row 0 survives
            f = f[:1] + 0.01 * f
        elif kind == "clusters":
            f = f[torch.arange(n, device=DEV) // 3 * 3] + 0.05 * f
        self.kind = kind
        self.inputs = {"features": f.contiguous()}
        self.outs = {"kept": 8 * n, "n_kept": 4}                 # int64[n], first *n_kept valid
        self.need = lib.hmm_gram_select_workspace_bytes(n)
        self.refusable = n > 2

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_gram_select(p["features"], self.n, 1024, C.c_float(0.9), p["kept"], p["n_kept"], ws, ws_bytes, None)

    def valid(self, raw):
        n = int(raw["n_kept"].view(torch.int32)[0])
        if self.n > 2:
            assert n == {"everything_kept": self.n, "nothing_kept": 1}.get(self.kind, n), (self.kind, n)
        return {"kept": 8 * n, "n_kept": 4}

    def shim(self):
        from hippomm_amd.consolidation import select_key_frames_device
        return {"kept": select_key_frames_device(self.inputs["features"], 0.9)}


# =====================================================================================================================
# encoder
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _tower(name):
    from hippomm_amd.encoder import HipTower
    from oracle import imagebind_oracle as ib
    spec = ib.reduced({"vision": ib.VISION_HUGE, "audio": ib.AUDIO_HUGE, "text": ib.TEXT_HUGE}[name], 2)
    return HipTower(name, ib.synthetic_state(spec, seed=1234, init="rich"), depth=2)


def _tower_input(name, batch):
    if name == "vision":
        return _rand((batch, 3, 224, 224), batch)
    if name == "audio":
        return _rand((batch, 3, 1, 128, 204), batch)
    g = torch.Generator().manual_seed(batch)
    tok = torch.randint(1, 49406, (batch, 77), generator=g)
    tok[torch.arange(batch), torch.randint(1, 77, (batch,), generator=g)] = 49407        # EOS: the largest id, where the head selects
    return tok.to(DEV)


# Which batch enters which regime (hmm_encoder_forward; splitk_mode / split_point / the fused-attention threshold in encoder.hip):
#   vision (257 tokens): 1 = split-K fc2 (<= 300 rows) | 2 = first batch outside it | 12 = last single chain | 13 = two half-batches
#     (6 + 7) | 47 = last unfused | 48 = first fused in_proj + attention | 64 = 16448 rows, the last forward whose few-row GEMMs may be
#     slivers | 65 = tiled kernels only.
#   audio (3 clips x 229 tokens): 1 = split-K (687 <= 700 rows) | 2 = outside it, unfused | 3 = fused from 9 clips | 4 = two chains from
#     12 clips | 5 and 7 = ONE chain again (15-21 clips x 12 heads <= 256 workgroups: one round) | 8 = two chains.
#   text (77 tokens): 1 and 9 = split-K (693 rows; the 9-question workspace is LARGER than the 10-question one) | 10 = outside it |
#     53 = last single chain | 54 = two half-batches.
ENCODER_BATCHES = {"vision": (1, 2, 12, 13, 47, 48, 64, 65), "audio": (1, 2, 3, 4, 5, 7, 8), "text": (1, 9, 10, 53, 54)}


class Encoder(Case):
    entry = "hmm_encoder_forward"

    def __init__(self, name, batch, streams=2, fused=1, ws_for=None):
        super().__init__()
        self.t, self.batch, self.streams, self.fused = _tower(name), batch, streams, fused
        self.family, self.label = f"encoder {name}", f"batch={batch},streams={streams},fused={fused}" + (f",ws_for={ws_for}" if ws_for else "")
        self.inputs = {"x": _tower_input(name, batch)}
        self.outs = {"out": 4096 * batch}
        self._settings()                                         # the size query answers for the handle's CURRENT stream setting
        self.need = self.t._lib.hmm_encoder_workspace_bytes(self.t._h, ws_for or batch)

    def _settings(self):
        self.t.set_streams(self.streams)
        self.t.set_fused_attention(self.fused)

    def call(self, lib, p, ws, ws_bytes):
        self._settings()
        return lib.hmm_encoder_forward(self.t._h, p["x"], self.batch, p["out"], ws, ws_bytes, None)

    def shim(self):
        self._settings()
        return {"out": self.t(self.inputs["x"], max_batch=self.batch)}


# =====================================================================================================================
# preprocessing: vision resize, audio fbank, SSIM, JPEG
# =====================================================================================================================
class Vision(Case):
    entry, family = "hmm_preprocess_vision_u8", "vision resize"

    def __init__(self, h, w, batch, window=False):
        super().__init__()
        from hippomm_amd import preprocess as pp
        _, lib = _L()
        self.h, self.w, self.B, self.window = h, w, batch, window
        frames = torch.randint(0, 256, (batch, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(h + w)).to(DEV)
        kh, bh, kv, bv, r0, r1 = pp._plan(h, w)
        if window:                                              # frames uploaded as the needed_window cut-out only
            x0, y0, ww, wh = pp.needed_window(h, w)
            frames = frames[:, y0:y0 + wh, x0:x0 + ww].contiguous()
            bh, bv = bh.copy(), bv.copy()
            bh[:, 0] -= x0
            bv[:, 0] -= y0
            r0, r1 = 0, wh
        self.in_h, self.in_w, self.r0, self.r1, self.ksh, self.ksv = frames.shape[1], frames.shape[2], r0, r1, kh.shape[1], kv.shape[1]
        self.label = f"{w}x{h},B={batch},rows[{r0},{r1}) of {self.in_h}" + (",window" if window else "")
        self.inputs = {"frames": frames, **{n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in
                                            (("kh", kh), ("bh", bh), ("kv", kv), ("bv", bv))}}
        self.outs = {"out": batch * 3 * 224 * 224 * 4}
        self.need = lib.hmm_preprocess_vision_workspace_bytes(batch, r1 - r0)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_preprocess_vision_u8(p["frames"], self.B, self.in_h, self.in_w, p["kh"], p["bh"], self.ksh, p["kv"], p["bv"],
                                            self.ksv, self.r0, self.r1, p["out"], ws, ws_bytes, None)

    def shim(self):
        from hippomm_amd import preprocess as pp
        out = torch.empty(self.B, 3, 224, 224, dtype=torch.float32, device=DEV)
        return {"out": pp._preprocess_into(self.inputs["frames"], out, (self.h, self.w) if self.window else None)}


class Fbank(Case):
    entry, family = "hmm_audio_fbank", "audio fbank"

    def __init__(self, n, clip_len, gap=0, tables=True):
        super().__init__()
        from hippomm_amd import preprocess as pp
        _, lib = _L()
        self.n, self.len, self.stride, self.tables = n, clip_len, clip_len + gap, tables
        self.label = f"clips={n},len={clip_len},stride={self.stride},tables={'supplied' if tables else 'generated'}"
        self.clips = 0.1 * _rand((n, clip_len), 5 + clip_len) + 0.01
        if tables:
            win, banks = pp._fbank_tables(DEV)
            self.inputs = {"window": win, "banks": banks}
        self.outs = {"out": n * 128 * 204 * 4}
        self.need = lib.hmm_audio_fbank_workspace_bytes(n)

    def sizes(self):
        return super().sizes() + [4 * ((self.n - 1) * self.stride + self.len)]

    def place_inputs(self, ar):
        ptr = super().place_inputs(ar)
        # clip c at clips + c * stride, clip_len samples each: (n - 1) * stride + clip_len floats, the gaps left as poison
        v = ar.carve(4 * ((self.n - 1) * self.stride + self.len), "clips")
        for c in range(self.n if self.len else 0):
            v[4 * c * self.stride: 4 * (c * self.stride + self.len)] = self.clips[c].view(torch.uint8)
        ptr["clips"] = ar.address(v)
        return ptr

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_audio_fbank(p["clips"], self.n, self.len, self.stride, p.get("window"), p.get("banks"), C.c_float(-4.268),
                                   C.c_float(9.138), p["out"], ws, ws_bytes, None)

    def shim(self):
        from hippomm_amd import preprocess as pp
        if not self.tables or self.len == 0:                     # the shim always supplies tables and cannot pass an empty clip
            return {}
        return {"out": pp.melspec_clips_device(self.clips, -4.268, 9.138)}


class Gray(Case):
    entry, family = "hmm_gray_u8", "gray"

    def __init__(self, h, w, n, order="RGB"):
        super().__init__()
        self.h, self.w, self.n, self.order, self.label = h, w, n, order, f"{w}x{h},n={n},{order}"
        self.inputs = {"frames": torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(h * w)).to(DEV)}
        self.outs = {"gray": n * h * w, "minmax": 8 * n}

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_gray_u8(p["frames"], self.n, self.h, self.w, {"RGB": 0, "BGR": 1}[self.order], p["gray"], p["minmax"], None)

    def shim(self):
        from hippomm_amd.ssim import gray_frames
        gray, minmax = gray_frames(self.inputs["frames"], self.order, return_minmax=True)
        return {"gray": gray, "minmax": minmax}


class Ssim(Case):
    entry, family = "hmm_ssim_pairs", "ssim"

    def __init__(self, h, w, n_pairs, from_a):
        super().__init__()
        _, lib = _L()
        self.h, self.w, self.m, self.from_a, self.nf = h, w, n_pairs, from_a, 3
        self.label = f"{w}x{h},pairs={n_pairs},range={'of frame a' if from_a else '255'}"
        g = torch.Generator().manual_seed(h + w)
        base = torch.randint(0, 256, (1, h, w), generator=g)
        gray = (base + torch.randint(-20, 21, (self.nf, h, w), generator=g)).clamp(0, 255).to(torch.uint8).to(DEV)
        self.pairs = np.ascontiguousarray(np.random.default_rng(n_pairs).integers(0, self.nf, (n_pairs, 2)), dtype=np.int32)
        self.inputs = {"gray": gray}
        if from_a:
            from hippomm_amd.ssim import gray_into
            minmax = torch.empty((self.nf, 2), dtype=torch.int32, device=DEV)
            gray_into(gray, 2, None, minmax)
            self.inputs["minmax"] = minmax
        self.outs = {"scores": 8 * n_pairs}
        self.need = lib.hmm_ssim_pairs_workspace_bytes(h, w, n_pairs)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_ssim_pairs(p["gray"], self.nf, self.h, self.w, self.pairs.ctypes.data, self.m,
                                  -1.0 if self.from_a else 255.0, p.get("minmax"), p["scores"], ws, ws_bytes, None)

    def shim(self):
        from hippomm_amd.ssim import ssim_pairs
        return {"scores": ssim_pairs(self.inputs["gray"], self.pairs, None if self.from_a else 255.0)}


def _jpeg_file(w, h, sub, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), ((x + y) * 3) % 256], axis=-1).astype(np.int32)
    img = np.clip(img + rng.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    img[: max(h // 5, 1), : max(w // 6, 1)] = (255, 0, 255)      # saturated patches push the colour conversion into its clamps
    img[h - max(h // 5, 1):, w - max(w // 6, 1):] = (0, 255, 0)
    im = Image.fromarray(img)
    buf = io.BytesIO()
    if sub == "grey":
        im.convert("L").save(buf, "JPEG", quality=90)
    else:
        im.save(buf, "JPEG", quality=90, subsampling=sub)
    return buf.getvalue()


class Jpeg(Case):
    entry = "hmm_jpeg_reconstruct"

    def __init__(self, w, h, sub, n, window=None):
        super().__init__()
        from hippomm_amd import jpeg
        _, lib = _L()
        self.window = tuple(window or (0, 0, w, h))
        self.n = n
        self.family = "jpeg " + {0: "4:4:4", 1: "4:2:2", 2: "4:2:0", "grey": "grey"}[sub]
        self.label = f"{w}x{h},n={n},window={self.window}"
        files = [_jpeg_file(w, h, sub, 100 * w + s) for s in range(n)]
        self.geometry = jpeg.parse(files[0])
        assert self.geometry is not None
        self.sb = jpeg.slot_bytes(self.geometry, self.window)
        slots = np.zeros((n, self.sb), dtype=np.uint8)
        for i, data in enumerate(files):
            assert jpeg.decode_coefs(data, self.geometry, self.window, slots[i]) == jpeg.DECODED
        self.g = jpeg._geom_array(self.geometry)
        self.inputs = {"slots": torch.from_numpy(slots).to(DEV)}             # n slots at stride slot_bytes: exactly n * slot_bytes
        self.outs = {"rgb": n * self.window[2] * self.window[3] * 3}
        self.need = lib.hmm_jpeg_workspace_bytes(self.g.ctypes.data, n, *self.window)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_jpeg_reconstruct(p["slots"], self.n, self.sb, self.g.ctypes.data, *self.window, p["rgb"], ws, ws_bytes, None)

    def shim(self):
        from hippomm_amd import jpeg
        out = torch.empty(self.n, self.window[3], self.window[2], 3, dtype=torch.uint8, device=DEV)
        return {"rgb": jpeg.reconstruct(self.inputs["slots"], self.geometry, self.window, out)}


# =====================================================================================================================
# building blocks without a workspace (assertions 1-4; the reference is the same call on ordinary torch buffers)
# =====================================================================================================================
class LayerNormOp(Case):
    entry, family = "hmm_op_layernorm_bf16", "op layernorm"

    def __init__(self, rows, D):
        super().__init__()
        self.rows, self.D, self.label = rows, D, f"rows={rows},D={D}"
        self.inputs = {"x": _rand((rows, D), rows + D), "gamma": _rand((D,), 1), "beta": _rand((D,), 2)}
        self.outs = {"y": rows * D * 2}

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_op_layernorm_bf16(p["x"], p["gamma"], p["beta"], p["y"], self.rows, self.D, 1e-6, None)

    def shim(self):
        y = torch.empty(self.rows, self.D, dtype=torch.bfloat16, device=DEV)
        i = self.inputs
        assert self.call(_L()[1], {"x": i["x"].data_ptr(), "gamma": i["gamma"].data_ptr(), "beta": i["beta"].data_ptr(), "y": y.data_ptr()}, None, 0) == 0
        return {"y": y}


class AttentionOp(Case):
    family = "op attention"

    def __init__(self, batch, tokens, heads, dh, bias_kv=False, causal=False):
        super().__init__()
        self.a = (batch, tokens, heads, dh)
        self.entry = "hmm_op_attention_causal_bf16" if causal else "hmm_op_attention_bf16"
        self.causal, self.label = causal, f"B={batch},T={tokens},H={heads},dh={dh}" + (",bias_kv" if bias_kv else "")
        D = heads * dh
        self.inputs = {"qkv": _rand((batch * tokens, 3 * D), tokens, torch.bfloat16)}
        if bias_kv:
            self.inputs.update(bias_k=_rand((D,), 3), bias_v=_rand((D,), 4))
        self.outs = {"out": batch * tokens * D * 2}

    def call(self, lib, p, ws, ws_bytes):
        if self.causal:
            return lib.hmm_op_attention_causal_bf16(p["qkv"], p["out"], *self.a, None)
        return lib.hmm_op_attention_bf16(p["qkv"], p["out"], *self.a, p.get("bias_k"), p.get("bias_v"), None)

    def shim(self):
        out = torch.empty(self.outs["out"] // 2, dtype=torch.bfloat16, device=DEV)
        p = {k: v.data_ptr() for k, v in self.inputs.items()}
        p["out"] = out.data_ptr()
        assert self.call(_L()[1], p, None, 0) == 0
        return {"out": out}


class StageOp(Case):
    """One of the tower-stage entry points (tests/test_gpu_stage_ops.py) on the inputs of one of that module's cases: every
    buffer at its exact size.  For hmm_op_gather_rows and hmm_op_layernorm_strided_bf16 the source ends with the last byte of
    the last row read, not at a whole stride."""
    family = "op stage"

    def __init__(self, entry, label, inputs, outs, args):
        super().__init__()
        self.entry, self.label, self.outs, self.args = entry, label, outs, args
        self.inputs = {k: v.to(DEV) for k, v in inputs.items()}

    def call(self, lib, p, ws, ws_bytes):
        return getattr(lib, self.entry)(*self.args(p), None)

    def shim(self):
        bufs = {name: torch.empty(nb, dtype=torch.uint8, device=DEV) for name, nb in self.outs.items()}
        p = {k: v.data_ptr() for k, v in {**self.inputs, **bufs}.items()}
        assert self.call(_L()[1], p, None, 0) == 0
        return bufs


def _stage_ops():
    import stage_cases as S
    pick = lambda stage, label: next(c for c in S.cases(stage) if c.label == label)
    iv, ia, fo, em = pick("im2col_vision", "n_img=1"), pick("im2col_audio", "n_clip=1"), pick("fold_conv3d", "D=5"), pick("embed_tokens", "batch=3")
    ga, asm = pick("gather_rows", "row=2560,T=229,n=3"), pick("assemble_tokens", "both,T=229,D=1280,n_img=2")
    eos, l2 = pick("layernorm_eos", "T=77,D=1024"), pick("l2norm_rows", "n_out=5,clips=3,scale=log20")
    at = [pick("attention_cls", "B=3,T=229,H=12,dh=64,bias=True,scale=1.0"), pick("attention_cls", "B=2,T=257,H=16,dh=80,bias=False,scale=1.0")]
    rows, T, D = 3, 5, 1280
    xs = _rand((((rows - 1) * T + 1) * D,), 5)
    ops = [
        StageOp("hmm_op_im2col_vision_bf16", iv.label, {"frames": iv.frames}, {"out": 256 * 640 * 2}, lambda p: (p["frames"], p["out"], 1)),
        StageOp("hmm_op_im2col_audio_bf16", ia.label, {"mels": torch.nan_to_num(ia.mels, nan=1.0)}, {"out": 228 * 256 * 2},
                lambda p: (p["mels"], p["out"], 1)),
        StageOp("hmm_op_fold_conv3d_bf16", fo.label, {"w": fo.w}, {"dst": 5 * 640 * 2}, lambda p: (p["w"], p["dst"], 5)),
        StageOp("hmm_op_assemble_tokens", asm.label, {"patches": asm.patches, "cls": asm.cls, "pos": asm.pos, "sg": asm.stem[0], "sb": asm.stem[1],
                                                      "pg": asm.pre[0], "pb": asm.pre[1]}, {"x": asm.n_img * asm.T * asm.D * 4},
                lambda p: (p["patches"], p["cls"], p["pos"], p["sg"], p["sb"], 1e-5, p["pg"], p["pb"], 1e-6, p["x"], asm.n_img, asm.T, asm.D)),
        StageOp("hmm_op_layernorm_strided_bf16", f"rows={rows},stride={T}x{D}", {"x": xs, "gamma": _rand((D,), 1), "beta": _rand((D,), 2)},
                {"y": rows * D * 2}, lambda p: (p["x"], T * D, p["gamma"], p["beta"], p["y"], rows, D, 1e-6)),
        StageOp("hmm_op_gather_rows", ga.label, {"src": ga.src}, {"dst": ga.n_rows * ga.row_bytes},
                lambda p: (p["src"], ga.stride, p["dst"], ga.n_rows, ga.row_bytes)),
        StageOp("hmm_op_embed_tokens", em.label, {"ids": em.ids, "table": em.table, "pos": em.pos}, {"x": em.n_rows * 1024 * 4},
                lambda p: (p["ids"], p["table"], p["pos"], p["x"], em.n_rows, em.T, em.vocab)),
        StageOp("hmm_op_layernorm_eos_bf16", eos.label, {"x": eos.x, "ids": eos.ids, "gamma": eos.gamma, "beta": eos.beta}, {"y": eos.B * eos.D * 2},
                lambda p: (p["x"], p["ids"], eos.T, p["gamma"], p["beta"], p["y"], eos.B, eos.D, 1e-6)),
        StageOp("hmm_op_l2norm_rows", l2.label, {"v": torch.nan_to_num(l2.v, nan=1.0), "log_scale": l2.log_scale}, {"out": l2.n_out * 1024 * 4},
                lambda p: (p["v"], p["out"], l2.n_out, l2.clips, p["log_scale"])),
    ]
    for c in at:
        ins = {"q": c.q, "kv": c.kv} | ({"bias_k": c.bk, "bias_v": c.bv} if c.bk is not None else {})
        ops.append(StageOp("hmm_op_attention_cls_bf16", c.label, ins, {"out": c.B * c.H * c.dh * 2},
                           lambda p, c=c: (p["q"], p["kv"], p["out"], c.B, c.T, c.H, c.dh, p.get("bias_k"), p.get("bias_v"))))
    return ops


class HotOp(StageOp):
    """One of the encoder's hot entry points (GEMM by named route, split-K and the LayerNorm that reduces it, the fused in_proj +
    attention kernels).  ``inout``: buffers the call reads AND writes (the fp32 residual stream); they are outputs of the case,
    carved like any output, and hold their initial value instead of the poison when the call starts."""
    family = "op hot"

    def __init__(self, entry, label, inputs, outs, args, inout=None):
        super().__init__(entry, label, inputs, outs, args)
        self.inout = {k: v.to(DEV) for k, v in (inout or {}).items()}
        self._ar = None

    def place_inputs(self, ar):
        self._ar = ar
        return super().place_inputs(ar)

    def call(self, lib, p, ws, ws_bytes):
        if self._ar is not None:                                    # in the arena: the initial value into the carved in/out buffer
            for name, t in self.inout.items():
                flat = _u8_dev(t)
                off = p[name] - self._ar.bytes.data_ptr()
                assert flat.numel() == self.outs[name] and 0 <= off <= self._ar.bytes.numel() - flat.numel()
                self._ar.bytes[off: off + flat.numel()].copy_(flat)
        return super().call(lib, p, ws, ws_bytes)

    def shim(self):
        bufs = {name: torch.empty(nb, dtype=torch.uint8, device=DEV) for name, nb in self.outs.items()}
        for name, t in self.inout.items():
            bufs[name].copy_(_u8_dev(t))
        p = {k: v.data_ptr() for k, v in {**self.inputs, **bufs}.items()}
        ar, self._ar = self._ar, None
        try:
            assert super().call(_L()[1], p, None, 0) == 0
        finally:
            self._ar = ar
        return bufs


def _u8_dev(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _hot_ops():
    """hmm_op_gemm_bf16_tile at a ragged M, one shape per kind of launch, over the four epilogues; split-K with four splits and
    the LayerNorm that reduces its slabs; the fused in_proj + attention kernels of the vision (3 images) and audio (5 clips) towers."""
    _, lib = _L()
    ops = []
    gemm_routes = [  # label, M, N, K, tile: the launches are pinned by tests/test_cpu_gemm_cases.py through hmm_op_gemm_plan
        ("sliver", 77, 256, 256, 5), ("ring", 77, 256, 256, 7), ("ring + sliver peel", 1283, 3072, 128, -2),
        ("ping-pong, guarded last row tile", 300, 256, 128, 3), ("ping-pong + peeled tail", 3077, 5120, 128, -1)]
    for what, M, N, K, tile in gemm_routes:
        a, w, bias = _rand((M, K), M, torch.bfloat16), _rand((N, K), N + K, torch.bfloat16) * 0.05, _rand((N,), 3)
        for epi in (0, 1, 2, 3):
            size = 2 if epi < 2 else 4
            ops.append(HotOp("hmm_op_gemm_bf16_tile", f"{what}: M={M},N={N},K={K},epi={epi},tile={tile}", {"a": a, "w": w, "bias": bias},
                             {"c": M * N * size}, lambda p, s=(M, N, K, epi, tile): (p["a"], p["w"], p["bias"], p["c"], *s),
                             inout={"c": _rand((M, N), 11)} if epi == 2 else None))
    M, N, K, splits = 77, 1024, 1024, 4
    a, w = _rand((M, K), 5, torch.bfloat16), _rand((N, K), 6, torch.bfloat16) * 0.05
    ops.append(HotOp("hmm_op_gemm_bf16_splitk", f"M={M},N={N},K={K},splits={splits}", {"a": a, "w": w}, {"part": splits * M * N * 4},
                     lambda p: (p["a"], p["w"], p["part"], M, N, K, splits, -1)))
    ops.append(HotOp("hmm_op_layernorm_reduce_bf16", f"rows={M},D={N},splits={splits}",
                     {"part": _rand((splits, M, N), 7), "bias": _rand((N,), 8), "gamma": _rand((N,), 1), "beta": _rand((N,), 2)},
                     {"x": M * N * 4, "y": M * N * 2},
                     lambda p: (p["x"], p["part"], splits, p["bias"], p["gamma"], p["beta"], p["y"], M, N, 1e-6),
                     inout={"x": _rand((M, N), 9)}))
    n_img, T, D = 3, 257, 1280
    a, w, bias = _rand((n_img * T, D), 21, torch.bfloat16), _rand((3 * D, D), 22, torch.bfloat16) * 0.03, _rand((3 * D,), 23) * 0.1
    cls_rows = a.view(n_img, T, D)[:, 0].contiguous()
    qkv_cls = torch.empty(n_img, 3 * D, dtype=torch.bfloat16, device=DEV)
    assert lib.hmm_op_gemm_bf16(cls_rows.data_ptr(), w.data_ptr(), bias.data_ptr(), qkv_cls.data_ptr(), n_img, 3 * D, D, 0, None) == 0
    torch.cuda.synchronize()
    ops.append(HotOp("hmm_op_qkv_attention_bf16", f"n_img={n_img}", {"a": a, "w": w, "bias": bias, "qkv_cls": qkv_cls},
                     {"out": n_img * T * D * 2}, lambda p: (p["a"], p["w"], p["bias"], p["qkv_cls"], p["out"], n_img)))
    n_clips, T, D = 5, 229, 768
    a, w, bias = _rand((n_clips * T, D), 31, torch.bfloat16), _rand((3 * D, D), 32, torch.bfloat16) * 0.04, _rand((3 * D,), 33) * 0.1
    ops.append(HotOp("hmm_op_qkv_attention_audio_bf16", f"n_clips={n_clips}",
                     {"a": a, "w": w, "bias": bias, "bias_k": _rand((D,), 34) * 0.5, "bias_v": _rand((D,), 35) * 0.5},
                     {"out": n_clips * T * D * 2}, lambda p: (p["a"], p["w"], p["bias"], p["bias_k"], p["bias_v"], p["out"], n_clips)))
    return ops


# =====================================================================================================================
# the case table
# =====================================================================================================================
# hmm_cosine_topk: the (n, k) list of tests/test_gpu_scan.py::test_matches_oracle (every path of run_scan: n <= 4096; fused with the
# one-kernel finish; fused with chunk passes, k in 65..128; the sims-buffer path, k > 128; the full bitonic sort, k > 1024) -- k > n
# and odd n are in it -- and a store with zero-norm rows.
SCAN_NK = [(1, 1), (1, 5), (2, 5), (63, 5), (4096, 32), (4097, 32), (8191, 7), (20000, 1), (20000, 5), (20000, 100), (20000, 1024),
           (9000, 2000), (5000, 5000), (70001, 32), (4097, 1), (4098, 64), (4104, 65), (12345, 128), (12345, 129), (300001, 64),
           (300001, 100)]
RAGGED_SMALL = [1, 3, 7, 64, 65, 200, 1, 1023, 2, 300]            # 1666 rows in 10 events: the 1024-key kernel; prefilter taken (>= 128 rows / event)
RAGGED_LARGE = [1, 5000, 4097, 12000, 2]                            # events beyond one 4096-key piece
RAGGED_TINY = [1, 2, 3, 50, 0, 7]                                   # fewer than 128 rows per event: the prefilter call IS the exact one

CASES = {
    "scan": lambda: [Scan(n, k) for n, k in SCAN_NK] + [Scan(4099, 5, "zero_rows"), Scan(333, 400, "zero_rows")],
    "scan_keys": lambda: [ScanKeys(n, k) for n, k in [(63, 5), (3, 8), (4097, 32), (12345, 129), (70001, 32), (9000, 2000)]],
    "prefilter": lambda: [Prefilter(40000, 32, "ties", "fallback"), Prefilter(20001, 5, "random", "prefilter"),
                          Prefilter(70001, 64, "random", "prefilter"), Prefilter(5000, 5, "random", "exact"),
                          Prefilter(20000, 100, "random", "exact")],
    "shadow_build": lambda: [ShadowBuild(n) for n in (1, 2, 5, 4097, 20001)],
    "segmented": lambda: [Segmented(RAGGED_SMALL, 5, False), Segmented(RAGGED_LARGE, 64, False), Segmented(RAGGED_LARGE, 100, False),
                          Segmented(RAGGED_TINY, 5, False), Segmented([1], 5, False)],
    "segmented_prefilter": lambda: [Segmented(RAGGED_SMALL, 5, True), Segmented(RAGGED_LARGE, 64, True), Segmented(RAGGED_LARGE, 100, True),
                                    Segmented(RAGGED_TINY, 5, True), Segmented([130], 200, True)],
    "multi": lambda: [Multi(63, 1, 5), Multi(3, 2, 5), Multi(1000, 16, 5), Multi(20001, 16, 5), Multi(20001, 17, 64),
                      Multi(5000, 3, 65), Multi(4097, 17, 1)],
    "merge_keys": lambda: [MergeKeys([5, 5], 16), MergeKeys([100, 7, 300], 64)],
    "rank_hits": lambda: [RankHits([1, 3, 7, 64], 5, 5), RankHits([2, 1], 5, 64), RankHits([30] * 900, 5, 5)],
    "gram": lambda: [Gram(n, "everything_kept") for n in (1, 2, 31, 32, 33, 255, 257, 3600)] +
                    [Gram(n, "nothing_kept") for n in (33, 257)] + [Gram(n, "clusters") for n in (31, 255, 3600)],
    "vision": lambda: [Vision(360, 640, 1), Vision(360, 640, 5), Vision(640, 360, 5), Vision(224, 224, 1), Vision(720, 1280, 5, window=True)],
    "fbank": lambda: [Fbank(1, 0), Fbank(7, 399), Fbank(1, 400), Fbank(7, 32000), Fbank(1, 40000), Fbank(7, 32000, gap=37),
                      Fbank(7, 401, gap=1), Fbank(1, 32000, tables=False), Fbank(7, 32000, gap=37, tables=False)],
    "gray": lambda: [Gray(7, 7, 1), Gray(8, 9, 3, "BGR"), Gray(120, 160, 2), Gray(1080, 1920, 1)],
    "ssim": lambda: [Ssim(7, 7, 1, False), Ssim(7, 7, 129, True), Ssim(8, 9, 129, True), Ssim(8, 9, 1, False), Ssim(120, 160, 128, False),
                     Ssim(120, 160, 129, True), Ssim(1080, 1920, 1, True), Ssim(1080, 1920, 129, False)],
    "jpeg": lambda: [Jpeg(w, h, sub, 1) for sub in (0, 1, 2, "grey") for w, h in ((1, 1), (15, 17), (130, 90))] +
                    # windows that start and end inside an MCU, and one-pixel windows in the corners (the chroma halo's clamps)
                    [Jpeg(130, 90, sub, 6, win) for sub in (0, 1, 2, "grey") for win in ((3, 5, 100, 70), (129, 89, 1, 1), (0, 0, 1, 1), (1, 1, 128, 88))] +
                    [Jpeg(1280, 720, 2, 1), Jpeg(1280, 720, 2, 6, (275, 0, 730, 720)), Jpeg(1280, 720, 1, 1, (9, 7, 1263, 705))],
    "ops": lambda: [LayerNormOp(1, 768), LayerNormOp(77, 1024), LayerNormOp(257, 1280), AttentionOp(1, 257, 16, 80),
                    AttentionOp(2, 229, 12, 64, bias_kv=True), AttentionOp(3, 77, 16, 64, causal=True)] + _hot_ops(),
    "stage_ops": _stage_ops,
}
# (5) X then Y in one workspace: another shape and another internal path
REUSE = {
    "scan": lambda: [(Scan(70001, 32), Scan(4097, 1)), (Scan(20000, 1024), Scan(12345, 128)), (Scan(9000, 2000), Scan(63, 5)),
                     (Scan(12345, 129), Scan(4104, 65)), (Scan(4104, 65), Scan(20000, 5))],
    "scan_keys": lambda: [(ScanKeys(12345, 129), ScanKeys(4097, 32)), (ScanKeys(4097, 32), ScanKeys(63, 5))],
    "prefilter": lambda: [(Prefilter(40000, 32, "ties", "fallback"), Prefilter(20001, 5, "random", "prefilter")),
                          (Prefilter(20001, 5, "random", "prefilter"), Prefilter(40000, 32, "ties", "fallback")),
                          (Prefilter(40000, 32, "ties", "fallback"), Prefilter(5000, 5, "random", "exact"))],
    "segmented": lambda: [(Segmented(RAGGED_LARGE, 64, False), Segmented(RAGGED_SMALL, 5, False)),
                          (Segmented(RAGGED_SMALL, 5, False), Segmented(RAGGED_LARGE, 100, False))],
    "segmented_prefilter": lambda: [(Segmented(RAGGED_LARGE, 64, True), Segmented(RAGGED_SMALL, 5, True)),
                                    (Segmented(RAGGED_SMALL, 5, True), Segmented(RAGGED_TINY, 5, True))],
    "multi": lambda: [(Multi(20001, 17, 64), Multi(63, 1, 5)), (Multi(5000, 3, 65), Multi(20001, 16, 5))],
    "gram": lambda: [(Gram(3600, "clusters"), Gram(33, "everything_kept")), (Gram(257, "nothing_kept"), Gram(255, "clusters"))],
    "vision": lambda: [(Vision(360, 640, 5), Vision(640, 360, 5)), (Vision(720, 1280, 5, window=True), Vision(224, 224, 1))],
    "fbank": lambda: [(Fbank(7, 32000), Fbank(1, 32000, tables=False)), (Fbank(1, 40000, tables=False), Fbank(7, 399))],
    "ssim": lambda: [(Ssim(1080, 1920, 129, False), Ssim(7, 7, 129, True)), (Ssim(8, 9, 129, True), Ssim(120, 160, 128, False))],
    "jpeg": lambda: [(Jpeg(1280, 720, 2, 1), Jpeg(15, 17, 0, 1)), (Jpeg(130, 90, "grey", 6, (3, 5, 100, 70)), Jpeg(130, 90, 1, 1))],
}


@pytest.mark.parametrize("group", list(CASES))
def test_guards_poison_independence_shim_extent_refusal(group):
    failures = []
    for case in CASES[group]():
        try:
            check_case(case)
        except AssertionError as exc:                             # every case of the group reports, not only the first
            failures.append(f"{case}: {exc}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("group", list(REUSE))
def test_reuse_of_one_workspace_across_shapes(group):
    failures = []
    for x, y in REUSE[group]():
        try:
            check_reuse(x, y)
        except AssertionError as exc:
            failures.append(f"{x} then {y}: {exc}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(ENCODER_BATCHES))
def test_encoder_every_regime(name):
    """Assertions 1-4 and 6 at the batches on both sides of every regime change (see ENCODER_BATCHES), two streams and one, fused
    attention on and off; the workspace is exactly hmm_encoder_workspace_bytes(batch)."""
    for batch in ENCODER_BATCHES[name]:
        ref = None
        for streams in (2, 1):
            for fused in ((1, 0) if name != "text" else (1,)):
                got = check_case(Encoder(name, batch, streams, fused))
                if ref is None:
                    ref = got
                _same(ref, got, f"encoder {name} batch {batch}: streams={streams} fused={fused} against the default")


@pytest.mark.parametrize("name", list(ENCODER_BATCHES))
def test_encoder_one_workspace_sized_for_the_largest_batch_serves_every_smaller_one(name):
    """The header's promise, and (5): every batch, largest first and then smallest first, in ONE workspace of
    hmm_encoder_workspace_bytes(largest) bytes that is never re-poisoned; results equal the fresh-workspace ones."""
    batches = ENCODER_BATCHES[name]
    top = max(batches)
    cases = {b: Encoder(name, b, ws_for=top) for b in batches}
    want = {b: fresh(Encoder(name, b), "ones")[0] for b in batches}
    need = cases[top].need
    assert all(c.need == need for c in cases.values())
    assert all(Encoder(name, b).need <= need for b in batches), "hmm_encoder_workspace_bytes is not non-decreasing"
    for pattern in ("ones", "big"):
        ar = A.GuardedArena(A.needed_bytes([s for c in cases.values() for s in c.sizes()]), DEV, A.PATTERNS[pattern])
        ws = ar.carve(need, "workspace")
        runs = {b: Run(cases[b], ar, ws=ws) for b in batches}
        for b in sorted(batches, reverse=True) + sorted(batches):
            for v in runs[b].out.values():
                ar.repoison(v)                                    # the outputs, not the workspace
            assert runs[b].launch(need) == 0
            ar.check_guards()
            _same(want[b], runs[b].results(), f"encoder {name} batch {b} in the workspace of batch {top} ({pattern})")
