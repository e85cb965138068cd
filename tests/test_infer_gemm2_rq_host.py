"""What infer_fuse_plan (csrc/infer.h) marks for k_infer_gemm2_i8_rq, without a GPU, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/support/infer_gemm2_rq_host.cpp, a stand-alone program, plans three models and prints the chains. The expected lines are worked out by hand
from the order of the ops (one per node; a QKV node is three products, an Mha node product, Softmax, product):
transformer_block: LayerNorm 0, Requant 1, QKV 2-4, Requants 5-7, Q K^T 8, Requant 9, Softmax 10, probabilities x V 11, Requant 12, ... (16 ops);
mha_block: ... Requants 5-7, Q K^T 8 (read by the Softmax: no chain), Softmax 9, probabilities x V 10, Requant 11, ... (15 ops).
Flags: 32 wide store (every stride a multiple of 16), 64 the Softmax is made in the kernel, 128 its table is staged in LDS (at most 2^14 entries),
256 a masked element is 0 (neg_inf = ((bkm >> 16) + 1) << 16 lies beyond bkm: the table gives 0)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "infer_gemm2_rq_host.cpp")


def test_the_marked_chains_and_the_masked_constant(tmp_path):
    import deep_prove_amd as dpa
    tb, mha, odd = dpa.models.transformer_block(64, 16, 2, 32, config=140), dpa.models.mha_block(16, 16, 4, 128, config=140), dpa.models.transformer_block(16, 16, 2, 16, config=142)
    odd.nodes[9][0]["left"] = (0, 1, 2)  # (the second product reads the probabilities transposed: planes in a layout the Softmax form does not admit)
    tv_tb, tv_mha = tb.nodes[8][0]["table_size"], mha.nodes[6][0]["table_size"]
    assert tv_tb <= 14 and tv_mha == 15 and odd.nodes[9][0]["kind"] == dpa.models.L_CONCAT_MATMUL
    want = ["model 0 ops 16", "gemm2 8 rq 9 flags 32 softmax -1 back 0 masked 0 table16 0", "gemm2 11 rq 12 flags 480 softmax 10 back 12 masked 0 table16 %d" % (2 << tv_tb),
            "model 1 ops 15", "gemm2 8 rq -1 flags 0 softmax -1 back 0 masked 0 table16 0", "gemm2 10 rq 11 flags 352 softmax 9 back 11 masked 0 table16 65536",
            "model 2 ops 16", "gemm2 8 rq 9 flags 32 softmax -1 back 0 masked 0 table16 0", "gemm2 11 rq -1 flags 0 softmax -1 back 0 masked 0 table16 0", "infer_gemm2_rq_host ok: 3 models"]
    args = []
    for name, mb in (("tb", tb), ("mha", mha), ("odd", odd)):
        np.ascontiguousarray(mb.blob(), dtype=np.int64).tofile(str(tmp_path / name))
        args.append(str(tmp_path / name))
    exe = tmp_path / "infer_gemm2_rq_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split("\n")[:-1] == want, r.stdout[-1500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
