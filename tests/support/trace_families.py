"""The model families of the trace-row tests (tests/test_trace_row.py, tests/test_gpu_zzzzzzzzzzzzz_trace.py and its child process): small
models that between them hold every kind of tensor a trace row carries — chains and graphs, a Conv node (whose FFT tables trace_from_row
makes again), a Flatten node, Embeddings with a learned positional table, a QKV node (three output slots, two model outputs), ConcatMatMul,
an Mha node (roles 16 and 17), LayerNorm, GELU and a Logits node (whose row maxima are derived). Where tests/golden/ holds a proof stream of
the family (mlp_w8.npz, cnn_tiny.npz, graph_models.json) the arguments are those of the golden case, and its input is builder.input()."""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# (name, arguments, keywords) of the builders in deep_prove_amd.models
FAMILIES = [("mlp", (2, 8), dict(config=9)),
            ("cnn_tiny", (), {}),
            ("token_mlp", (16, 50, 32), dict(config=71, max_positions=40)),
            ("attention_block", (), dict(seq=8, emb=16, heads=2, head_dim=8, config=61)),
            ("mha_block", (), dict(seq=8, emb=16, heads=2, head_dim=8, config=97)),
            ("gelu_mlp", (), dict(width=256, config=112)),
            ("qkv_two_outputs", (), dict(seq=4, k=16, n=16, config=64)),
            ("logits_only", (4, 8), dict(config=5)),
            ("lm_head", (4, 16, 32), dict(config=13))]
IDS = [f[0] for f in FAMILIES]
NEEDS_ALL_KINDS = {"mha_block", "gelu_mlp"}


def build(family):
    import deep_prove_amd as dpa
    name, args, kw = family
    return getattr(dpa.models, name)(*args, **kw)


def inputs(mb, n, first=1000):
    """n inputs of the builder; row 0 is builder.input(), the input of the golden streams"""
    return np.stack([mb.input(first + i) for i in range(n)])


def golden_proof_sha256(family):
    """sha256 of the committed proof stream of (family, builder.input()), or None when tests/golden/ has none"""
    name, args, kw = family
    g = os.path.join(ROOT, "tests", "golden")
    if name in ("mlp", "cnn_tiny"):
        z = np.load(os.path.join(g, "mlp_w8.npz" if name == "mlp" else "cnn_tiny.npz"))
        mb = build(family)
        assert (z["model_blob"] == mb.blob()).all() and (z["input"] == mb.input()).all()
        return hashlib.sha256(np.ascontiguousarray(z["proof"], dtype=np.uint64).tobytes()).hexdigest()
    with open(os.path.join(g, "graph_models.json")) as f:
        for c in json.load(f):
            if c["model"] == name and c["args"] == kw and not args:
                return c["proof_sha256"]
    return None
