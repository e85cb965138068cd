"""One rank of a sharded sumcheck between PROCESSES (tests/test_gpu_zzzzzzzzzzz_peer_exchange.py, tools/peer_exchange_probe.py):

    peer_child.py <dir> <rank> <world> <nv> [repeats]

The rank builds ITS slice of three base tables of 2^nv entries (models.splitmix64, the tables of tests/golden/sumcheck24.json), creates its peer group, writes
the group's handle to <dir>/handle_<rank> (write, then rename), waits for every rank's handle, connects, proves the product of the three tables together with
its peers and writes proof_<rank>.npy, finals_<rank>.npy and next_<rank>.json (the next challenge of its transcript). It then writes done_<rank> and waits for
every done_* before it frees its mailbox: nobody frees while a peer may still post to it. With `repeats`, the proof is repeated and the median milliseconds go
to ms_<rank>.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
P = 0xFFFFFFFF00000001
NTABLES = 3
WAIT_S = 60.0


def full_table(nv, j):
    import deep_prove_amd as dpa
    return dpa.models.splitmix64(0xD33B0000 ^ (5 << 32) ^ j, 1 << nv) % np.uint64(P)


def _publish(path, data):
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


def _await(paths, what):
    deadline = time.monotonic() + WAIT_S
    while not all(os.path.exists(p) for p in paths):
        if time.monotonic() > deadline:
            raise SystemExit(f"{what}: not all there after {WAIT_S:.0f} s")
        time.sleep(0.005)


def main():
    d, rank, world, nv = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    import deep_prove_amd as dpa
    chunk = (1 << nv) // world
    dev = dpa.Device(0)
    tabs = [dpa.Mle.from_base(dev, np.ascontiguousarray(full_table(nv, j)[rank * chunk:(rank + 1) * chunk])) for j in range(NTABLES)]
    terms = [((1, 0), list(range(NTABLES)))]
    group = dpa.sharded.PeerGroup(dev, rank, world)
    _publish(os.path.join(d, f"handle_{rank}"), group.handle)
    paths = [os.path.join(d, f"handle_{g}") for g in range(world)]
    _await(paths, "handles")
    group.connect([open(p, "rb").read() for p in paths])
    t = dpa.Transcript(b"test")
    proof, finals = dpa.sharded.prove_sharded_peer(dev, group, nv, tabs, terms, t)
    np.save(os.path.join(d, f"proof_{rank}.npy"), proof)
    np.save(os.path.join(d, f"finals_{rank}.npy"), finals)
    _publish(os.path.join(d, f"next_{rank}.json"), json.dumps({"next_challenge": list(t.read_challenge()), "fine_grained": group.fine_grained}).encode())
    if repeats:
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            again, _ = dpa.sharded.prove_sharded_peer(dev, group, nv, tabs, terms, dpa.Transcript(b"test"))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert (again == proof).all()
        _publish(os.path.join(d, f"ms_{rank}.json"), json.dumps({"ms": ms}).encode())
    _publish(os.path.join(d, f"done_{rank}"), b"1")
    _await([os.path.join(d, f"done_{g}") for g in range(world)], "done marks")
    group.close()
    for m in tabs:
        m.free()
    dev.close()


if __name__ == "__main__":
    main()
