"""CPU: the planted-relation inputs of select_relation_cases.py, independent of any kernel.  The tests check the inputs, not the
kernels: the modelled relation is the planted one, every cosine is far from the threshold, the closed-form kept lists are what
the exact definition and the model give under every partition the GPU tests use, each mutant of the model is caught by a planted
case, and the mutants that stand for the gap (far tiles, columns from 2048 on, last kept tile only) change nothing on the inputs
the select tests had before."""
import numpy as np
import pytest

import keyframe_stream_cases as K
import recipes
import select_relation_cases as R
from oracle.consolidation_oracle import select_key_frames_exact


@pytest.mark.parametrize("name", R.CASES)
def test_modelled_relation_is_the_planted_one_with_margin(name):
    f, thr, planted, _ = R.case(name)
    cos, rel = R.case_model(name)
    n = f.shape[0]
    assert planted.shape == (n, n) and planted.dtype == bool and np.array_equal(planted, planted.T)
    assert np.array_equal(rel, planted)
    off = ~np.eye(n, dtype=bool)
    if np.isfinite(thr):                          # an infinite or NaN threshold decides every pair without looking at the value
        gap = np.abs(cos[off & np.isfinite(cos)] - float(np.float32(thr)))
        assert gap.min() >= R.MARGIN, gap.min()
    assert np.all(planted[np.isnan(cos)])          # a NaN cosine is a hit whatever the threshold
    weakest, strongest = R.cosine_stats(name)
    print(f"{name}: n={n} thr={thr} weakest planted cosine {weakest}, strongest unplanted cosine {strongest}")


@pytest.mark.parametrize("name", R.CASES)
def test_closed_form_kept_list_is_the_exact_definition_and_the_model(name):
    f, thr, planted, want = R.case(name)
    n = f.shape[0]
    assert want[0] == 0 and want == sorted(set(want)) and want[-1] < n
    assert select_key_frames_exact(f, thr).tolist() == want
    assert R.one_shot(planted) == want
    for label, part in R.partitions(name, n).items():
        assert part[0][0] == 0 and part[-1][1] == n and all(p[1] == q[0] for p, q in zip(part, part[1:]))
        model = K.ModelSelector(similarity_threshold=thr)
        for a, b in part:
            model.extend(f[a:b])
            assert model.kept() == K.expected_after(want, b), (label, b)
        seen = []
        assert R.grown(planted, part, after_each=lambda b, kept: seen.append(kept == K.expected_after(want, b))) == want
        assert all(seen) and len(seen) == len(part), label


def test_the_cases_reach_what_they_are_for():
    _, _, rel, _ = R.case("matching_n320")
    assert R.tile_pairs_hit(rel) == {(ti, tj) for ti in range(5) for tj in range(ti, 5)}       # all 15 tile pairs
    _, pairs = R.matching_pairs(2113, 2113, R.EXPLICIT_2113)
    assert len(pairs) == len(R.EXPLICIT_2113) + 2113 // 4 and len({r for p in pairs for r in p}) == 2 * len(pairs)
    _, _, rel, _ = R.case("matching_n2113")
    assert all(rel[i, j] and rel[j, i] for i, j in R.EXPLICIT_2113)
    assert len(R.tile_pairs_hit(rel)) > 300                                                     # of the 34 * 35 / 2 = 595
    for v in R.GRID_LAST:
        pairs = R.kept_grid_pairs(v)
        assert len({k for k, _ in pairs}) == len({j for _, j in pairs}) == len(pairs)           # every hit decides its own row
        cells = {(k // R.TILE, (j - R.GRID_KEPT) // R.TILE) for k, j in pairs}
        assert {c for c in cells if c[1] < 2} == {(kt, nt) for kt in range(5) for nt in range(2)}
        assert {kt for kt, nt in cells if nt == 2} == set(R.GRID_LAST[v])
        in_tile = {k % R.TILE for k, _ in pairs} | {(j - R.GRID_KEPT) % R.TILE for _, j in pairs}
        assert {0, 31, 32, 63} <= in_tile
        assert R.GRID_KEPT - 1 in {k for k, _ in pairs}                                         # the row a partial tile pads with
    assert {kt for v in R.GRID_LAST for kt in R.GRID_LAST[v]} == set(range(5))                  # the 5 x 3 grid, between them


def _outcomes(name, mutant):
    """{route: kept list} of a planted case under a mutant of the model."""
    _, _, rel, _ = R.case(name)
    out = {"one-shot": R.one_shot(rel, mutant)}
    for label, part in R.partitions(name, rel.shape[0]).items():
        out[label] = R.grown(rel, part, mutant)
    return out


CATCHES = [("far_tiles", "matching_n320", "one-shot"), ("far_tiles", "matching_n320", "all"),
           ("word64", "matching_n2113", "one-shot"), ("word64", "matching_n2113", "all"),
           ("dropped_block", "non_transitive", "one-shot"), ("dropped_block", "non_transitive", "all"),
           ("last_kept_tile", "kept_grid_a", "cycle+130"), ("last_kept_tile", "kept_grid_b", "cycle+130"),
           ("last_kept_tile", "kept_grid_c", "cycle+130"), ("last_kept_tile", "matching_n320", "64"),
           ("diag_tile_only", "kept_grid_a", "cycle+130"), ("diag_tile_only", "matching_n320", "all"),
           ("diag_tile_only", "matching_n320", "100")]


@pytest.mark.parametrize("mutant,name,route", CATCHES)
def test_each_mutant_is_caught_by_a_planted_case(mutant, name, route):
    assert mutant in R.MUTANTS
    assert _outcomes(name, mutant)[route] != R.case(name)[3]
    assert _outcomes(name, None)[route] == R.case(name)[3]


def test_every_mutant_is_listed_as_caught():
    assert {m for m, _, _ in CATCHES} == set(R.MUTANTS)


def test_a_hit_in_any_grid_cell_is_seen_only_by_looking_at_that_kept_tile():
    """The last-kept-tile mutant keeps exactly the copies whose original lies in kept tiles 0..3."""
    for v in R.GRID_LAST:
        _, _, rel, want = R.case(f"kept_grid_{v}")
        got = _outcomes(f"kept_grid_{v}", "last_kept_tile")["cycle+130"]
        assert sorted(set(got) - set(want)) == sorted(j for k, j in R.kept_grid_pairs(v) if k // R.TILE < 4)


def _tile_edge_input():
    """The input of test_gpu_keyframe_stream.py::test_kept_count_crosses_tile_edges and its partition."""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((130, 1024)).astype(np.float32)
    edge = [0, 63, 64, 127, 128, 129]
    copies = np.concatenate([base[edge], base[edge] * np.float32(2.5)])
    fresh = rng.standard_normal((1, 1024)).astype(np.float32)
    return np.concatenate([base, copies, fresh]), K.batches(130, K.CYCLE) + [(i, i + 1) for i in range(130, 143)]


ORACLE_INPUTS = [(100, 20, 0.2, 0.9), (1000, 150, 0.25, 0.9), (777, 90, 0.3, 0.9), (500, 60, 0.2, 0.5), (500, 60, 0.2, 0.97),
                 (65, 65, 0.0, 0.9), (2049, 300, 0.2, 0.9)]                 # test_gpu_select.py::test_matches_oracle


def test_the_gap_mutants_change_nothing_on_the_older_inputs():
    """Far tiles, columns from 2048 on, last kept tile only: on every recipes.SELECT_CASES input, under the partitions of the
    stream tests, and on the clustered inputs of test_matches_oracle the mutated model lists what the real one lists.  The one
    older input that tells two of them apart is test_kept_count_crosses_tile_edges'."""
    for name in recipes.SELECT_CASES:
        f, _ = recipes.select_case(name)
        rel = R.relation(f, 0.9)
        assert R.one_shot(rel) == K.GOLD[name], name
        for mutant in ("far_tiles", "word64"):
            assert R.one_shot(rel, mutant) == K.GOLD[name], (name, mutant)
        for label, part in K.partitions(name, f.shape[0]).items():
            for mutant in ("far_tiles", "word64", "last_kept_tile"):
                assert R.grown(rel, part, mutant) == K.GOLD[name], (name, label, mutant)
    for n, clusters, sigma, thr in ORACLE_INPUTS:
        rel = R.relation(recipes.clustered(n, clusters, sigma, seed=n + clusters), thr)
        for mutant in ("far_tiles", "word64"):
            assert R.one_shot(rel, mutant) == R.one_shot(rel), (n, mutant)
    f, part = _tile_edge_input()
    rel = R.relation(f, 0.9)
    want = list(range(130)) + [142]
    assert R.one_shot(rel) == R.grown(rel, part) == want
    assert R.one_shot(rel, "far_tiles") != want and R.grown(rel, part, "last_kept_tile") != want
    assert R.one_shot(rel, "word64") == R.grown(rel, part, "word64") == R.grown(rel, part, "far_tiles") == want
