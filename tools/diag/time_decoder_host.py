"""What the decoders' Python host layer costs per call, this tree against another checkout of the repository (the parent
commit's, built), alternating -- also in who goes first --, ROUNDS rounds each, every leg in a fresh process:
    python3 tools/diag/time_decoder_host.py PATH_OF_THE_OTHER_BUILT_TREE
(a) the decode numbers of `bench.py --full` (bench.decode_numbers, without the CPU baselines): greedy at B=1024 T=1500 V=29,
    beam 100 at B=64 T=1500 V=29 without and with the synthetic 3-gram, all through CTCDecoderEngine -- wall ms of the engine call;
(b) the wall time of feed_nbest on each of the three engines' streams where the host dominates: B=2, chunks of 5 frames,
    beam_width 4, no model, 200 calls after 20 warm-up calls (a call ends in the read-out's copy to the host, so the clock stops
    behind the kernel); the stream is reset, untimed, every 10 chunks -- median and mean us per call.
A figure of this tree passes if it lies inside the other tree's own spread over its rounds, or is faster.
DECODER_HOST_JSON=path: also write the numbers there (profiles/decoder_host/)."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROUNDS, WARMUP, CALLS = 3, 20, 200
B, CHUNK, W, MAX_FRAMES = 2, 5, 4, 50


def worker(root):
    sys.path.insert(0, root)
    import torch
    import bench
    from end2end_amd import engines as E
    assert os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))) == os.path.abspath(root), E.__file__
    dev = torch.device("cuda", 0)
    res = {}
    for k, v in bench.decode_numbers(dev, False).items():
        if k in ("greedy", "beam100", "beam100_lm"):
            res["bench_%s_ms" % k] = v["ms"]
    g = torch.Generator().manual_seed(7)
    chars = [chr(97 + i) for i in range(26)] + [" ", "'"]
    streams = {
        "ctc": (E.CTCDecoderEngine(0, W, ["_"] + chars).open_stream(B, MAX_FRAMES),
                torch.log_softmax(torch.randn(B, MAX_FRAMES, 29, generator=g, dtype=torch.float64) * 3, -1).float().to(dev)),
        "asg": (E.ASGBeamEngine(chars, 0, W).open_stream(torch.randn(28, 28, generator=g), B, MAX_FRAMES),
                torch.randn(B, MAX_FRAMES, 28, generator=g).to(dev)),
        "gram": (E.GramCTCDecoderEngine(0, 5, 7, {5: [1, 2], 6: [3, 4, 1]}, W, ["_", "a", "b", "c", " "]).open_stream(B, MAX_FRAMES),
                 torch.log_softmax(torch.randn(B, MAX_FRAMES, 7, generator=g, dtype=torch.float64) * 3, -1).float().to(dev)),
    }
    for name, (st, x) in streams.items():
        ts = []
        for i in range(WARMUP + CALLS):
            at = (i * CHUNK) % MAX_FRAMES
            if at == 0:
                st.reset()
                torch.cuda.synchronize()
            chunk = x[:, at:at + CHUNK]
            t0 = time.perf_counter()
            r = st.feed_nbest(chunk)
            ts.append(time.perf_counter() - t0)
            assert len(r[2]) == B and st.frames == [at + CHUNK] * B
        ts = [t * 1e6 for t in ts[WARMUP:]]
        res["feed_nbest_%s_median_us" % name] = statistics.median(ts)
        res["feed_nbest_%s_mean_us" % name] = statistics.fmean(ts)
    print("RESULT " + json.dumps(res))


def main(other):
    trees = {"parent": os.path.abspath(other), "branch": HERE}
    runs = {k: [] for k in trees}
    for r in range(ROUNDS):
        for k, root in (list(trees.items()) if r % 2 == 0 else list(trees.items())[::-1]):   # (who goes first alternates too)
            p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--worker", root],
                               capture_output=True, text=True, cwd=root)
            line = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("round %d, %s: exit status %d\n%s\n%s" % (r, k, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            runs[k].append(json.loads(line[0][len("RESULT "):]))
            print("round %d %-6s %s" % (r, k, "  ".join("%s %.1f" % (n.replace("feed_nbest_", "").replace("bench_", ""), v)
                                                        for n, v in runs[k][-1].items())), flush=True)
    record = {"shape": "bench.decode_numbers; feed_nbest: B=%d, chunks of %d frames, beam_width %d, no model, %d calls after %d"
                       % (B, CHUNK, W, CALLS, WARMUP), "rounds": ROUNDS, "figures": {}}
    for n in runs["parent"][0]:
        pa, br = [x[n] for x in runs["parent"]], [x[n] for x in runs["branch"]]
        verdict = "inside" if min(pa) <= statistics.median(br) <= max(pa) else "faster" if statistics.median(br) < min(pa) else "slower"
        record["figures"][n] = {"parent": [round(v, 2) for v in pa], "branch": [round(v, 2) for v in br],
                                "branch_median_against_parent_spread": verdict}
        print("%-32s parent %s  branch %s  %s" % (n, record["figures"][n]["parent"], record["figures"][n]["branch"], verdict))
    if os.environ.get("DECODER_HOST_JSON"):
        os.makedirs(os.path.dirname(os.environ["DECODER_HOST_JSON"]), exist_ok=True)
        with open(os.environ["DECODER_HOST_JSON"], "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    elif len(sys.argv) == 2:
        main(sys.argv[1])
    else:
        sys.exit(__doc__)
