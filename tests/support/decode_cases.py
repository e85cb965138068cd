"""Shared by tests/test_decode_host.py and tests/test_gpu_zzzzzzzzzzzzzz_decode.py: the two decodable model families, and greedy decoding as a
numpy loop over ModelBuilder.run — the expectation of both files, independent of the library."""
import numpy as np

EOS, WINDOW, MAX_NEW, REFUSED = 1, 2, 3, 4
SEQ, VOCAB = 8, 16


def gelu_lm():
    """Embeddings, a constant addend, Linear, Requant, GELU, the head, Requant, Logits: needs all_kinds on the device"""
    import deep_prove_amd as dpa
    return dpa.models.token_lm(SEQ, VOCAB, 16, config=43)


def relu_lm():
    """the same with ReLU and a learned positional table twice as long as the window: needs no flag"""
    import deep_prove_amd as dpa
    return dpa.models.token_lm(SEQ, VOCAB, 16, config=48, gelu=False, max_positions=16)


FAMILIES = [("gelu_lm", gelu_lm, True), ("relu_lm", relu_lm, False)]  # (name, builder, needs all_kinds)
IDS = [f[0] for f in FAMILIES]


def numpy_decode(mb, prompt, prompt_len, max_new, eos=None, pad=0):
    """(tokens[seq], length, stop, output[seq]): every step tests the limits, runs the model on the whole padded window and takes the token at
    length - 1; the end-of-sequence token is not appended; the output is the model's on the final tokens"""
    seq = mb.input_len
    tokens = np.full(seq, pad, dtype=np.int64)
    tokens[:prompt_len] = np.asarray(prompt, dtype=np.int64)[:prompt_len]
    length = prompt_len
    while True:
        if length == seq:
            stop = WINDOW
            break
        if length == prompt_len + max_new:
            stop = MAX_NEW
            break
        t = int(mb.run(tokens)[length - 1])
        if eos is not None and t == eos:
            stop = EOS
            break
        tokens[length] = t
        length += 1
    return tokens, length, stop, np.asarray(mb.run(tokens), dtype=np.int64)


def prompts(mb, n):
    """n full windows of tokens, [n][seq]: prompt i is row i cut to its prompt_len"""
    return np.stack([mb.input(1000 + s) for s in range(n)])
