#!/usr/bin/env python3
"""Generate tests/golden/checkpoint_golden.json by running the UNMODIFIED reference's _save_checkpoint.

Run in the build container only (it needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_checkpoint_golden.py [--reference DIR]

HippocampalMemory._save_checkpoint (hippomm/core/hippocampal_memory.py:1486-1524) is imported behind the stub modules of
make_golden.py and called unchanged on a ``HippocampalMemory.__new__`` object that has only ``storage_dir`` set, with the
reference's own ShortTermMemory / SequenceSegment objects built from the recipe of tests/checkpoint_cases.py.  Only the recipe,
the timestamp read back from the file and the file's text are written.
"""
from __future__ import annotations

import argparse
import json
import platform
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import checkpoint_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference checkout (default: where make_golden.py looks)")
    a = ap.parse_args()
    import make_golden
    if a.reference:
        make_golden.REF = a.reference
    make_golden.import_reference()
    import hippomm.core.hippocampal_memory as hm

    memories = K.recipe_memories(K.RECIPE, memory=hm.ShortTermMemory, segment=hm.SequenceSegment)
    with tempfile.TemporaryDirectory() as tmp:
        self = hm.HippocampalMemory.__new__(hm.HippocampalMemory)
        self.storage_dir = Path(tmp)
        path = hm.HippocampalMemory._save_checkpoint(self, K.RECIPE["video_id"], memories)
        if path is None:
            raise SystemExit("the reference's _save_checkpoint returned None")
        text = Path(path).read_text()
        name = Path(path).name
    data = json.loads(text)
    out = {"_generated_by": "tests/golden/make_checkpoint_golden.py",
           "_env": {"numpy": np.__version__, "python": platform.python_version()},
           "_reference": {"save": "hippomm/core/hippocampal_memory.py:1486-1524", "to_dict": "hippomm/core/hippocampal_memory.py:56-92"},
           "recipe": K.RECIPE, "file_name_pattern": name.replace(str(int(data["timestamp"])), "{int(now)}"),
           "timestamp": data["timestamp"], "text": text}
    K.GOLDEN.write_text(json.dumps(out, indent=1))
    same = K.expected_text(K.RECIPE["video_id"], K.recipe_memories(), data["timestamp"]) == text.encode("ascii")
    print(f"{K.GOLDEN}: {K.GOLDEN.stat().st_size} bytes; file text {len(text)} bytes; the helper's expression reproduces it: {same}")
    if not same:
        raise SystemExit("tests/checkpoint_cases.expected_text does not reproduce the reference's file")


if __name__ == "__main__":
    main()
