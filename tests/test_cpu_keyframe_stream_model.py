"""CPU: the decomposition behind hmm_keyframe_extend, independent of any kernel.  A numpy model of the five steps (hit bits from an
fp64 gram rounded once to fp32, new x kept bits seeding a greedy scan of each batch, n <= 2 read-out) is fed every select fixture
under the batch partitions and must list, after every batch, the golden kept list restricted to the rows seen."""
import numpy as np
import pytest

import keyframe_stream_cases as K
import recipes
from oracle.consolidation_oracle import select_key_frames_exact

CASES = recipes.SELECT_CASES + recipes.SELECT_INBAND_CASES


@pytest.mark.parametrize("name", CASES)
def test_model_reproduces_the_golden_prefix_after_every_batch(name):
    f, _ = recipes.select_case(name)
    assert recipes.sha256(f) == K.SHA[name]
    n = f.shape[0]
    parts = K.partitions(name, n)
    if name == "n3600_clusters600":
        parts["cycle"] = K.batches(n, K.CYCLE)               # cheap on the host: the model runs the long input under more
        parts["33"] = K.batches(n, [33])
        parts["all"] = K.batches(n, [n])
    for label, part in parts.items():
        model = K.ModelSelector()
        for a, b in part:
            model.extend(f[a:b])
            assert model.n_seen == b
            assert model.kept() == K.expected_after(K.GOLD[name], b), (label, b)
            if n <= 70:
                assert model.kept() == select_key_frames_exact(f[:b]).tolist(), (label, b)
        assert model.kept() == K.GOLD[name], label


def test_two_identical_rows_are_both_listed_until_a_third_arrives():
    v = np.random.default_rng(3).standard_normal((1, 1024)).astype(np.float32)
    model = K.ModelSelector()
    model.extend(v)
    model.extend(v)
    assert model.kept() == [0, 1] and model.kept_idx == [0]
    model.extend(np.random.default_rng(4).standard_normal((1, 1024)).astype(np.float32))
    assert model.kept() == [0, 2]


def test_partitions_cover_every_row_once():
    for n in (1, 2, 3, 64, 65, 257, 3600):
        for part in K.partitions("x", n).values():
            assert part[0][0] == 0 and part[-1][1] == n
            assert all(a < b for a, b in part) and all(p[1] == q[0] for p, q in zip(part, part[1:]))
