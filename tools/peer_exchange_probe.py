"""What does the peer exchange cost per round, next to the thread exchange it stands beside?

    python tools/peer_exchange_probe.py [out=profiles/peer_exchange.txt]

For W in {2, 4} ranks on ONE GPU and a 2^16 sumcheck (three base tables, one product: latency-bound, every local round is a launch, an exchange and a wait),
ten proofs each, alternating in one call:
  A  dp_sumcheck_prove_sharded_local — W contexts, one library thread per rank, the in-process exchange (two host barriers, two stream synchronisations and
     device-to-device copies per round, then k_shares_sum_publish);
  B  W PeerGroup ranks, one Python thread per rank, dp_sumcheck_prove_peer — one k_peer_exchange_publish launch per round.
And W = 2 as two PROCESSES (tests/support/peer_child.py), which only B can do. Prints the median milliseconds per proof and the difference per local round.
There is no threshold: the figures are what they are on the box that ran this."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# W ranks of one process are W streams whose kernels wait for each other: each needs a hardware queue of its own (read when HIP initialises)
try:
    _queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "0"))
except ValueError:
    _queues = 0
if _queues < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
NV, REPS = 16, 10


def main():
    import deep_prove_amd as dpa
    import peer_child
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "peer_exchange.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    full = [peer_child.full_table(NV, j) for j in range(peer_child.NTABLES)]
    terms = [((1, 0), list(range(peer_child.NTABLES)))]
    d0 = dpa.Device(0)
    say(f"peer exchange probe: 2^{NV} sumcheck, {peer_child.NTABLES} base tables, one product; {REPS} proofs per variant, A and B alternating; device {d0.name}")
    d0.close()
    for world in (2, 4):
        k = world.bit_length() - 1
        chunk = (1 << NV) // world
        devs = [dpa.Device(0) for _ in range(world)]
        rows = [[dpa.Mle.from_base(d, np.ascontiguousarray(t[g * chunk:(g + 1) * chunk])) for t in full] for g, d in enumerate(devs)]
        groups = [dpa.sharded.PeerGroup(d, g, world) for g, d in enumerate(devs)]
        for g in groups:
            g.connect([h.handle for h in groups])

        def prove_a():
            t0 = time.perf_counter()
            proof, _ = dpa.sharded.prove_sharded_local(devs, NV, rows, terms, [dpa.Transcript(b"test") for _ in range(world)])
            return (time.perf_counter() - t0) * 1e3, proof

        def prove_b():
            res = [None] * world

            def rank(g):
                res[g] = dpa.sharded.prove_sharded_peer(devs[g], groups[g], NV, rows[g], terms, dpa.Transcript(b"test"))[0]
            th = [threading.Thread(target=rank, args=(g,), daemon=True) for g in range(world)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join(90.0)
            ms = (time.perf_counter() - t0) * 1e3
            if any(t.is_alive() for t in th) or any(r is None for r in res):
                raise SystemExit("a rank of the peer exchange did not come back")
            return ms, res[0]

        ref = prove_a()[1]
        assert (prove_b()[1] == ref).all(), "the two exchanges give different proofs"  # (and a warm-up of both)
        a, b = [], []
        for _ in range(REPS):
            ms, p = prove_a()
            a.append(ms)
            ms, p2 = prove_b()
            b.append(ms)
            assert (p == ref).all() and (p2 == ref).all()
        ma, mb = statistics.median(a), statistics.median(b)
        say(f"W = {world} (threads of one process), fine-grained mailbox exported: {groups[0].fine_grained}")
        say(f"  A thread exchange : median {ma:8.3f} ms per proof  (min {min(a):.3f}, max {max(a):.3f})")
        say(f"  B peer exchange   : median {mb:8.3f} ms per proof  (min {min(b):.3f}, max {max(b):.3f})")
        say(f"  B - A per local round ({NV - k} rounds): {(mb - ma) * 1e3 / (NV - k):+8.1f} us   (B starts its ranks as Python threads, A as library threads)")
        for g in groups:
            g.close()
        for row in rows:
            for m in row:
                m.free()
        for d in devs:
            d.close()
    # two processes
    world = 2
    with tempfile.TemporaryDirectory() as d:
        child = os.path.join(ROOT, "tests", "support", "peer_child.py")
        procs = [subprocess.Popen([sys.executable, child, d, str(g), str(world), str(NV), str(REPS)], cwd=ROOT) for g in range(world)]
        try:
            rcs = [p.wait(timeout=180) for p in procs]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        if any(rcs):
            raise SystemExit(f"the two-process run failed: {rcs}")
        ms = [json.load(open(os.path.join(d, f"ms_{g}.json")))["ms"] for g in range(world)]
        fine = json.load(open(os.path.join(d, "next_0.json")))["fine_grained"]
    per_proof = [max(ms[0][i], ms[1][i]) for i in range(REPS)]  # (a proof is done when its slower rank is)
    mp = statistics.median(per_proof)
    say(f"W = 2 (two processes, mailboxes mapped with hipIpcOpenMemHandle), fine-grained mailbox exported: {fine}")
    say(f"  B peer exchange   : median {mp:8.3f} ms per proof  (min {min(per_proof):.3f}, max {max(per_proof):.3f}); {mp * 1e3 / (NV - 1):.1f} us per local round, launch, exchange and host sponge included")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
