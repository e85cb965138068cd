"""Writes tests/golden/logits_models.json: for every Logits::Argmax case of tests/support/logits_cases.py the sha256 of the model blob, the input,
the output (the chosen tokens) and the proof stream, as little-endian words.

What this fixture pins: the product's HOST LOGIC over the plain-loop CPU double (tests/support/logits_check.cpp over tests/support/cpu_dev.hpp), not
the oracle. The other golden streams of this directory come from the oracle, an independent restatement of the reference; for layer kind 18 no
oracle restatement exists yet (follow-up), so the fixture can only say "the GPU build computes what
the host orchestrator computes over plain loops, and neither changes unnoticed". What makes the streams RIGHT is checked elsewhere: the product
verifier, its flip sweeps and forgeries (tests/test_logits_hostlogic.py) and the second, independent reading of the verifier (tests/test_logits_independent.py).
usage: python tests/golden/make_logits_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from support import logits_cases as LC  # noqa: E402

if __name__ == "__main__":
    binary, out = LC.check_bin(), {}
    with tempfile.TemporaryDirectory() as d:
        for name, (mb, x) in LC.cases().items():
            bp, xp = LC.write_case(d, name, mb.blob(), x)
            sp, op = os.path.join(d, name + ".stream"), os.path.join(d, name + ".out")
            r = LC.run_check(binary, "run", bp, xp, sp, op)
            assert r.returncode == 0, r.stdout + r.stderr
            stream, y = np.fromfile(sp, dtype="<u8"), np.fromfile(op, dtype="<i8")
            out[name] = dict(blob=LC.sha(mb.blob(), np.int64), input=LC.sha(x, np.int64), output=LC.sha(y, np.int64), stream=LC.sha(stream, np.uint64),
                             stream_words=int(stream.size), tokens=[int(v) for v in y])
    with open(LC.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", LC.GOLDEN)
