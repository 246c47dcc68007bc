#!/usr/bin/env python3
"""Same-box, same-process A/B of overlapped enqueues: two contexts on one stream, one created with
MCAMD_ENQUEUE_OVERLAP=0 (in order, as before) and one with MCAMD_ENQUEUE_OVERLAP=1, timed in alternating pairs.
    python3 tools/enqueue_ab.py [--pairs 15] [--steps 20]          # on an MI355X
Each timing is bench.py's own timed region: K back-to-back mcamd_price_paths_enqueue calls (fp64, 252 steps, a seed per
call) and one device-wide sync, by the host's wall clock.  Sizes: 10M paths (the headline), 100M and 5M.  The control is
the same two contexts timing synchronous mcamd_price_paths calls at 10M, which the variable must not move.  "ratio" is
overlap on / overlap off of the same pair.  The yardstick (profiles/pairsum_skew_ab.txt): a gain if every ratio at 10M is
below 1 and the whole range lies below the control's smallest ratio."""
import argparse, importlib, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAR = "MCAMD_ENQUEUE_OVERLAP"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    capi = importlib.import_module("monte-carlo-project-cuda_amd").capi
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctxs = {}
    for name, value in (("off", "0"), ("on", "1")):
        os.environ[VAR] = value   # read once, when the context is created
        ctxs[name] = capi.Context(0, stream.cuda_stream)
    del os.environ[VAR]
    opt = capi.make_option()
    K = args.steps
    stats = torch.zeros((K, 6), dtype=torch.float64, device="cuda")

    def enqueued(ctx, n, seed0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            ctx.price_paths_enqueue(opt, capi.make_sim(n, 252, capi.F64, seed0 + i), stats[i])
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / K
        return wall, sum(ctx.enqueued_kernel_ms(K)) / K

    def synchronous(ctx, n, seed0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            ctx.price_paths(opt, capi.make_sim(n, 252, capi.F64, seed0 + i))
        return (time.perf_counter() - t0) * 1e3 / K, 0.0

    med = lambda xs: sorted(xs)[len(xs) // 2]

    def table(title, run, n):
        for c in ctxs.values():   # warm both: clocks, code objects, scratch buffers, the internal streams
            for _ in range(2):
                run(c, n, 7)
        rows = {"off": [], "on": []}
        for p in range(args.pairs):
            for name in ("off", "on"):
                rows[name].append(run(ctxs[name], n, 1000 + 64 * p))
        ratios = [on[0] / off[0] for off, on in zip(rows["off"], rows["on"])]
        print(title)
        for name in ("off", "on"):
            w, k = [r[0] for r in rows[name]], [r[1] for r in rows[name]]
            print(f"   overlap {name:3s}  wall ms per job: median {med(w):8.4f}  min {min(w):8.4f}  max {max(w):8.4f}"
                  + (f"   reported kernel ms per job: median {med(k):8.4f}" if any(k) else "") + f"  (n={len(w)})")
        print(f"   ratio on / off per pair: median {med(ratios):.4f}  min {min(ratios):.4f}  max {max(ratios):.4f}"
              f"   pairs below 1: {sum(r < 1.0 for r in ratios)} of {len(ratios)}")
        print("   ratios: " + " ".join(f"{r:.4f}" for r in ratios))
        return ratios

    print(f"build id {capi.build_id()}, {ctxs['on'].device_info().name.decode()}, K = {K} jobs per timing, "
          f"{args.pairs} alternating pairs (off, on)")
    head = table(f"enqueue f64 10M x 252, {K} back to back + sync", enqueued, 10_000_000)
    table(f"enqueue f64 100M x 252, {K} back to back + sync", enqueued, 100_000_000)
    table(f"enqueue f64 5M x 252, {K} back to back + sync", enqueued, 5_000_000)
    ctrl = table(f"control: synchronous price_paths f64 10M x 252, {K} calls", synchronous, 10_000_000)
    gain = max(head) < 1.0 and max(head) < min(ctrl)
    print(f"10M: every ratio below 1: {max(head) < 1.0}; whole range ({min(head):.4f} - {max(head):.4f}) below the "
          f"control's minimum ({min(ctrl):.4f}): {max(head) < min(ctrl)}; counts as a gain: {gain}")
    for c in ctxs.values():
        c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
