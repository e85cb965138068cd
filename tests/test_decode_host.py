"""Decoding without a GPU (include/deep_prove_hip_decode.h): dp_model_decode_host against greedy decoding written as a numpy loop over
ModelBuilder.run (tests/support/decode_cases.py), the eligibility refusals and their messages, the relation dp_verify_decode checks before it
reads a proof, the ABI surface, and decode_step — the step the host loop and the kernel share — in a stand-alone program under AddressSanitizer
and UndefinedBehaviorSanitizer (tests/support/decode_step_host.cpp). Every comparison is exact equality."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deep_prove_hip_decode.h")
STEP_SRC = os.path.join(ROOT, "tests", "support", "decode_step_host.cpp")
C11 = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"]
ENTRIES = {"dp_model_decode": "int32_t (*)(dp_model*, const int64_t*, const uint32_t*, size_t, uint32_t, int64_t, int64_t, uint32_t, int64_t*, uint32_t*, uint32_t*, uint32_t*, int64_t*, double*)",
           "dp_model_decode_host": "int32_t (*)(const int64_t*, size_t, const int64_t*, uint32_t, uint32_t, int64_t, int64_t, int64_t*, uint32_t*, uint32_t*, uint32_t*, int64_t*)",
           "dp_verify_decode": "int32_t (*)(const uint64_t*, size_t, const uint64_t*, size_t, const int64_t*, size_t, const int64_t*, uint32_t, uint32_t, uint32_t, int64_t, int64_t, uint32_t)"}
sys.path.insert(0, os.path.join(ROOT, "tests"))
from support.decode_cases import EOS, FAMILIES, IDS, MAX_NEW, REFUSED, SEQ, VOCAB, WINDOW, gelu_lm, numpy_decode, prompts  # noqa: E402


def _same(got, want):
    tokens, length, stop, reason, out = got
    wt, wl, ws, wo = want
    return (tokens == wt).all() and length == wl and stop == ws and reason == 0 and (out == wo).all()


def test_the_cases_of_the_gelu_family_in_numbers():
    """the completions this family is known to give: prompts of two tokens, up to six new ones"""
    import deep_prove_amd as dpa
    mb = gelu_lm()
    blob, xs = mb.blob(), prompts(mb, 4)
    assert list(xs[0][:2]) == [13, 15] and list(xs[2][:2]) == [15, 12]
    dec = lambda s, eos: dpa.decode_host(blob, xs[s], 2, 6, eos=eos)
    assert list(dec(0, None)[0]) == [13, 15, 7, 10, 6, 9, 2, 10] and list(dec(2, None)[0]) == [15, 12, 5, 10, 6, 9, 2, 10]
    assert [dec(s, 9)[1:3] for s in range(4)] == [(5, EOS)] * 4
    assert [dec(s, 12)[1:3] for s in range(4)] == [(8, WINDOW), (2, EOS), (8, WINDOW), (2, EOS)]
    for s in range(4):
        for eos in (None, 9, 12):
            assert _same(dec(s, eos), numpy_decode(mb, xs[s], 2, 6, eos))


@pytest.mark.parametrize("name,make,_", FAMILIES, ids=IDS)
def test_decode_host_equals_the_numpy_loop(name, make, _):
    """prompt_len 1, 2, 7, 8 (8 = seq: WINDOW without an inference), max_new 0, 1, 6, eos none / 9 / 12 / a prompt token / the pad token"""
    import deep_prove_amd as dpa
    mb = make()
    blob, xs = mb.blob(), prompts(mb, 3)
    stops = set()
    for s in range(3):
        for plen in (1, 2, 7, 8):
            for max_new in (0, 1, 6):
                for eos, pad in ((None, 0), (9, 0), (12, 0), (int(xs[s][0]), 0), (3, 3), (0, 0)):
                    want = numpy_decode(mb, xs[s], plen, max_new, eos, pad)
                    got = dpa.decode_host(blob, xs[s][:plen], plen, max_new, eos=eos, pad=pad)
                    assert _same(got, want), (name, s, plen, max_new, eos, pad, got, want)
                    assert want[2] == (WINDOW if plen == 8 else MAX_NEW if max_new == 0 else want[2])
                    assert (got[0][got[1]:] == pad).all() and (got[0][:plen] == xs[s][:plen]).all()
                    stops.add(want[2])
    assert stops == {EOS, WINDOW, MAX_NEW}
    # prompt_len defaults to the whole prompt; a prompt token equal to eos stops nothing
    got = dpa.decode_host(blob, xs[0][:3], max_new=2, eos=int(xs[0][1]))
    assert _same(got, numpy_decode(mb, xs[0], 3, 2, int(xs[0][1]))) and got[1] >= 3


def test_a_refused_prompt_keeps_its_tokens():
    """a token outside the vocabulary: REFUSED with the class of the Embeddings refusal, the tokens and the length as they stood, zeros for the output"""
    import deep_prove_amd as dpa
    mb = gelu_lm()
    for plen, max_new in ((3, 4), (8, 0), (2, 0)):
        x = prompts(mb, 1)[0].copy()
        x[1] = VOCAB
        tokens, length, stop, reason, out = dpa.decode_host(mb.blob(), x[:plen], plen, max_new)
        assert stop == REFUSED and reason == 2 and length == plen and (tokens[:plen] == x[:plen]).all() and not tokens[plen:].any() and not out.any()


def _softmax_chain():
    """tokens -> Embeddings -> Softmax -> Logits: everything a decodable model needs, and a Softmax"""
    import deep_prove_amd as dpa
    mb = dpa.models.ModelBuilder((4,), 5)
    mb.embeddings(4, 4)
    mb.shape_og = mb.shape_pad = (1, 4, 4)
    mb.softmax()
    mb.shape_og = mb.shape_pad = (4, 4)
    return mb.logits()


def test_eligibility_refusals_and_their_messages():
    import deep_prove_amd as dpa
    good = gelu_lm().blob()
    cases = [(dpa.models.lm_head(8, 16, 16, config=3).blob(), dict(), "node 0 must be an Embeddings layer"),
             (dpa.models.token_mlp(8, 16, 16, config=3).blob(), dict(), "the only output of the model must be a Logits node"),
             (_softmax_chain().blob(), dict(), "holds a Softmax"),
             (good, dict(pad=VOCAB), "pad 16 lies outside the vocabulary of 16"),
             (good, dict(pad=-1), "pad -1 lies outside the vocabulary"),
             (good, dict(prompt_len=0), "prompt_len 0 of prompt 0 lies outside 1..8"),
             (good, dict(prompt_len=9), "prompt_len 9 of prompt 0 lies outside 1..8")]
    for blob, kw, message in cases:
        args = dict(prompt_len=2, max_new=3)
        args.update(kw)
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.decode_host(blob, [1, 2], **args)
        assert ei.value.code == -1 and str(ei.value).find("dp_model_decode: ") >= 0 and message in str(ei.value), str(ei.value)


def test_verify_decode_refuses_each_violation_of_the_relation():
    """the relation is checked before the proof is read: a one-word proof and a one-word verifier blob get as far as the proof check and no further"""
    import deep_prove_amd as dpa
    mb = gelu_lm()
    x = prompts(mb, 1)[0]
    dummy = np.zeros(1, dtype=np.uint64)

    def refused(message, tokens, out, plen, length, stop, eos=None, pad=0, max_new=6):
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.verify_decode(dummy, dummy, tokens, out, plen, length, stop, eos=eos, pad=pad, max_new=max_new)
        assert ei.value.code == -5 and "dp_verify_decode: " in str(ei.value) and message in str(ei.value), (message, str(ei.value))

    def reaches_the_proof(tokens, out, plen, length, stop, eos=None, pad=0, max_new=6):
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.verify_decode(dummy, dummy, tokens, out, plen, length, stop, eos=eos, pad=pad, max_new=max_new)
        assert "dp_verify_decode" not in str(ei.value), str(ei.value)

    tw, lw, sw, ow = numpy_decode(mb, x, 2, 6)          # fills the window
    te, le, se, oe = numpy_decode(mb, x, 2, 6, eos=9)   # EOS at length 5
    tm, lm, sm, om = numpy_decode(mb, x, 2, 2)          # MAX_NEW at length 4
    assert (lw, sw, le, se, lm, sm) == (8, WINDOW, 5, EOS, 4, MAX_NEW)
    reaches_the_proof(tw, ow, 2, 8, WINDOW)
    reaches_the_proof(te, oe, 2, 5, EOS, eos=9)
    reaches_the_proof(tm, om, 2, 4, MAX_NEW, max_new=2)
    # 1. the lengths
    refused("1 <= prompt_len <= length <= seq", tw, ow, 0, 8, WINDOW)
    refused("1 <= prompt_len <= length <= seq", tw, ow, 3, 2, WINDOW)
    refused("1 <= prompt_len <= length <= seq", tw, ow, 2, 9, WINDOW)
    # 2. an altered generated token (position 4 is the model's choice at position 3)
    bad = tw.copy()
    bad[4] = (bad[4] + 1) % VOCAB
    refused("token 4 is not the one the model chose at position 3", bad, ow, 2, 8, WINDOW)
    # 3. an end-of-sequence token among the appended ones: the first is chosen at position 1
    refused("the end-of-sequence token was chosen at position 1 and decoding went on", tw, ow, 2, 8, WINDOW, eos=int(tw[2]))
    reaches_the_proof(tw, ow, 2, 8, WINDOW, eos=int(tw[0]))  # (a prompt token equal to eos stops nothing: 13 is never chosen here)
    assert int(tw[0]) not in list(ow[1:7])
    # 4. a tail that is not pad
    bad = te.copy()
    bad[6] = 4
    refused("token 6 behind the completion is not the pad token", bad, oe, 2, 5, EOS, eos=9)
    refused("token 5 behind the completion is not the pad token", te, oe, 2, 5, EOS, eos=9, pad=1)
    # 5. each wrong stop claim
    refused("stop WINDOW claimed at length 5 of 8", te, oe, 2, 5, WINDOW, eos=9)
    refused("stop MAX_NEW claimed at length 5, prompt_len + max_new is 8", te, oe, 2, 5, MAX_NEW, eos=9)
    assert int(ow[7]) not in list(ow[1:7])  # (the token chosen at the last position is none of the appended ones: only the stop claim is wrong)
    refused("stop EOS claimed for a full window", tw, ow, 2, 8, EOS, eos=int(ow[7]))
    refused("stop EOS claimed at length 4 == prompt_len + max_new", tm, om, 2, 4, EOS, eos=int(om[3]), max_new=2)
    refused("stop EOS claimed, but the model chose", te, oe, 2, 5, EOS, eos=11)
    refused("stop EOS claimed, but the model chose", te, oe, 2, 5, EOS, eos=None)
    refused("stop MAX_NEW claimed for a full window", tw, ow, 2, 8, MAX_NEW)
    refused("stop WINDOW claimed at length 4 of 8", tm, om, 2, 4, WINDOW, max_new=2)
    refused("stop MAX_NEW claimed at length 4, prompt_len + max_new is 5", tm, om, 2, 4, MAX_NEW, max_new=3)
    refused("never verifiable", tw, ow, 2, 8, REFUSED)
    refused("unknown stop reason 0", tw, ow, 2, 8, 0)
    # a length one too small: the tail then starts at a generated token
    refused("token 4 behind the completion is not the pad token", te, oe, 2, 4, MAX_NEW, eos=9, max_new=2)


def test_header_is_strict_c11_and_a_c_program_links_against_the_three_symbols(tmp_path):
    import deep_prove_amd as dpa
    lib = ctypes.CDLL(dpa.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    src, out = tmp_path / "link.c", tmp_path / "link"
    body = "".join(f"  {{ {sig.replace('(*)', '(*f)')} = {name}; bad |= f == 0; }}\n" for name, sig in ENTRIES.items())
    src.write_text('#include "deep_prove_hip_decode.h"\nint main(void) {\n  int bad = DP_DECODE_STOP_EOS != 1u || DP_DECODE_STOP_WINDOW != 2u || DP_DECODE_STOP_MAX_NEW != 3u || DP_DECODE_STOP_REFUSED != 4u'
                   ' || DP_INFER_ALL_KINDS != 1u;\n' + body + "  return bad;\n}\n")
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
    d = os.path.dirname(dpa.LIB_PATH)
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-O1", "-o", str(out), str(src), "-L", d, "-ldeepprove_hip", "-lpthread", "-Wl,-rpath," + d])
    assert subprocess.run([str(out)]).returncode == 0


def test_the_other_headers_and_the_pinned_extern_block_do_not_mention_them():
    hdr = open(HEADER).read()
    main = open(os.path.join(ROOT, "include", "deep_prove_hip.h")).read()
    infer = open(os.path.join(ROOT, "include", "deep_prove_hip_infer.h")).read()
    for name in list(ENTRIES) + ["DP_DECODE_STOP"]:
        assert name in hdr and name not in main and name not in infer, name
    rs = os.path.join(ROOT, "rust", "deep-prove-hip-sys", "src")
    lib = open(os.path.join(rs, "lib.rs")).read()
    first = lib[lib.index('extern "C" {'):]
    first = first[:first.index("\n}")]
    decode_rs = open(os.path.join(rs, "decode.rs")).read()
    for name in ENTRIES:
        assert name + "(" not in first and f"pub fn {name}(" in decode_rs, name
    assert "mod decode;" in lib and "pub const DP_DECODE_STOP_REFUSED: u32 = 4;" in decode_rs


def test_python_surface():
    import importlib
    import deep_prove_amd as dpa
    mod = importlib.import_module("deep_prove_amd.infer")
    for name in ENTRIES:
        assert name in mod.DECODE_SIGNATURES and name not in mod.INFER_SIGNATURES and name not in dpa._lib.SIGNATURES, name
    assert [len(mod.DECODE_SIGNATURES[n][1]) for n in ENTRIES] == [14, 12, 13]
    assert (mod.STOP_EOS, mod.STOP_WINDOW, mod.STOP_MAX_NEW, mod.STOP_REFUSED) == (1, 2, 3, 4)
    assert callable(dpa.decode_host) and callable(dpa.verify_decode)
    for fn in (dpa.Context.decode, dpa.Prover.decode_and_prove):
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:4] == ["prompts", "prompt_lens", "max_new"] and sig["eos"].default is None and sig["pad"].default == 0 and sig["all_kinds"].default is False


def test_decode_step_under_sanitizers(tmp_path):
    """every (length, limit, eos, status, earlier stop, chosen token) at seq = 4 as a single step, and every small decode as a loop, with the token
    and output rows in heap blocks of exactly seq words"""
    exe = tmp_path / "decode_step_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), STEP_SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "decode_step_host ok: 10800 single steps, 2400 decodes" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
