#!/usr/bin/env python
"""Times of the LargeSteps solves on the GPU (DESIGN.md section "LargeSteps"; raw output under profiles/):

    python tools/smooth_bench.py [--out profiles/smooth_bench.txt] [--rounds 7]

  - time per solve of both launch forms on the four icospheres (42 / 642 / 2562 / 40962 vertices) at lambda = 19 and 100, cold and warm-started from a
    perturbed solution, against the same conjugate gradients in eager torch (index_add_ on the edge list): what a user would write without the library;
  - the crossover of the two forms: padded spheres up to the one-workgroup limit;
  - what the launches behind the raised `done` flag cost: the same solve with max_iter = its iteration count and with max_iter larger by 64 ... 1024
    (the host stops enqueuing at the first look that finds the flag up, so the count of such launches is read from info()).

Every figure is the median of `rounds` windows, the variants interleaved in one process, each window = enough solves for a few milliseconds, timed by device
events around the window.  Needs an MI355X: there is no CPU path."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "psdr-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import psdr_cuda  # noqa: E402
import smooth_cases as sc  # noqa: E402


def torch_cg(edges, deg, lam, b, x0, tol, max_iter):
    """The eager-torch conjugate gradients a user would write: M p by index_add_ on the directed edge list, three columns in lockstep, one test per iteration
    read on the host (the usual `if` on a residual).  Returns (x, iterations)."""
    def M(x):
        y = (1.0 + lam * deg).unsqueeze(1) * x
        return y.index_add_(0, edges[0], x[edges[1]], alpha=-lam)
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    r = b - M(x) if x0 is not None else b.clone()
    bb = (b * b).sum(0)
    rr = (r * r).sum(0)
    thr = tol * tol * bb
    p = r.clone()
    for k in range(max_iter):
        if bool((rr <= thr).all()):
            return x, k
        Ap = M(p)
        pAp = (p * Ap).sum(0)
        active = rr > thr
        alpha = torch.where(active & (pAp > 0), rr / pAp, torch.zeros_like(rr))
        x = x + alpha * p
        r = r - alpha * Ap
        rr_new = (r * r).sum(0)
        beta = torch.where(active & (rr_new > thr), rr_new / rr, torch.zeros_like(rr))
        p = r + beta * p
        rr = torch.where(active, rr_new, rr)
    return x, max_iter


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # microseconds per call


def measure(variants, rounds, target_us=20000.0):
    """variants: {name: fn}; returns {name: (median, min) microseconds per call}, the variants interleaved round by round"""
    reps = {}
    for k, fn in variants.items():
        fn(); fn()
        torch.cuda.synchronize()
        t = window(fn, 3)
        reps[k] = int(max(3, min(2000, target_us / max(t, 1.0))))
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(window(fn, reps[k]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two spheres, three rounds (a rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench.py needs a GPU: the solves have no CPU path")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    levels = (3, 4) if args.quick else (1, 3, 4, 6)
    rounds = 3 if args.quick else args.rounds
    say("# smooth_bench%s: %s, torch %s, rounds %d, %s" % (" --quick" if args.quick else "", torch.cuda.get_device_name(0), torch.__version__, rounds, time.strftime("%Y-%m-%d")))
    probe = psdr_cuda.LargeSteps(np.array([[0, 1, 2]], np.int32), 3)
    limit = probe.info()["one_workgroup_limit"]
    say("# one-workgroup limit %d vertices, default crossover %d, default max_iter %d" % (limit, probe.info()["one_workgroup_default"], probe.max_iter))

    say("\n## time per solve, microseconds (median / min); tol 1e-6, max_iter = the default")
    say("%-6s %7s %6s %5s | %5s %21s | %5s %21s | %5s %21s | %s" % ("mesh", "V", "lambda", "start", "iter", "one workgroup", "iter", "multi launch", "iter", "eager torch", "torch / best"))
    for level in levels:
        v, f = sc.icosphere(level)
        V = len(v)
        e = sc.unique_edges(V, f)
        edges = torch.as_tensor(np.concatenate([e, e[:, ::-1]]).T.copy(), device="cuda")
        deg = torch.zeros(V, device="cuda").index_add_(0, edges[0], torch.ones(edges.shape[1], device="cuda"))
        for lam in (19.0, 100.0):
            b = torch.as_tensor(np.random.default_rng(11).standard_normal((V, 3)).astype(np.float32), device="cuda")
            forms = {}
            if V <= limit:
                forms["one"] = psdr_cuda.LargeSteps(f, V, lmbda=lam, one_workgroup=1)
            forms["multi"] = psdr_cuda.LargeSteps(f, V, lmbda=lam, one_workgroup=0)
            exact = forms["multi"].from_differential(b)
            # warm start: the previous step's positions -- the solution moved by 1e-3 of its size, an Adam step's worth
            warm = exact + 1e-3 * exact.abs().mean() * torch.as_tensor(np.random.default_rng(5).standard_normal((V, 3)).astype(np.float32), device="cuda")
            for start, x0 in (("cold", None), ("warm", warm)):
                variants, iters = {}, {}
                for k, ls in forms.items():
                    variants[k] = (lambda ls=ls: ls.from_differential(b, x0=x0))
                    variants[k]()
                    iters[k] = ls.info()["iterations"]
                variants["torch"] = lambda: torch_cg(edges, deg, lam, b, x0, 1e-6, probe.max_iter)
                iters["torch"] = torch_cg(edges, deg, lam, b, x0, 1e-6, probe.max_iter)[1]
                t = measure(variants, rounds)
                best = min(t[k][0] for k in forms)
                cell = lambda k: ("%5d %9.1f / %9.1f" % (iters[k], t[k][0], t[k][1])) if k in t else "%5s %21s" % ("-", "-")
                say("ico%-3d %7d %6g %5s | %s | %s | %s | %.1fx" % (level, V, lam, start, cell("one"), cell("multi"), cell("torch"), t["torch"][0] / best))

    say("\n## crossover: an icosphere padded with isolated vertices, lambda = 19, cold; microseconds (median)")
    say("%7s | %5s %10s | %5s %10s" % ("V", "iter", "one wg", "iter", "multi"))
    for V in ((642, 2562) if args.quick else (162, 642, 1024, 1536, 2048, 2562, 3072, 3584, limit)):
        base = max(l for l in (1, 2, 3, 4) if len(sc.icosphere(l)[0]) <= V)
        v, f = sc.padded(*sc.icosphere(base), V)
        b = torch.as_tensor(np.random.default_rng(V).standard_normal((V, 3)).astype(np.float32), device="cuda")
        forms = {"one": psdr_cuda.LargeSteps(f, V, one_workgroup=1), "multi": psdr_cuda.LargeSteps(f, V, one_workgroup=0)}
        variants, iters = {}, {}
        for k, ls in forms.items():
            variants[k] = (lambda ls=ls: ls.from_differential(b))
            variants[k]()
            iters[k] = ls.info()["iterations"]
        t = measure(variants, rounds)
        say("%7d | %5d %10.1f | %5d %10.1f" % (V, iters["one"], t["one"][0], iters["multi"], t["multi"][0]))

    idle_level = 4 if args.quick else 6
    v, f = sc.icosphere(idle_level)
    V = len(v)
    say("\n## launches behind the raised `done` flag: ico%d (%d vertices), lambda = 19, cold, multi launch; microseconds per solve (median) by max_iter" % (idle_level, V))
    b = torch.as_tensor(np.random.default_rng(11).standard_normal((V, 3)).astype(np.float32), device="cuda")
    ls = psdr_cuda.LargeSteps(f, V, one_workgroup=0, max_iter=4096)
    ls.from_differential(b)
    need = ls.info()["iterations"]
    variants, solvers = {}, {}
    for extra in (0, 64, 256, 1024):
        solvers[extra] = psdr_cuda.LargeSteps(f, V, one_workgroup=0, max_iter=need + extra)
        variants[extra] = (lambda l=solvers[extra]: l.from_differential(b))
    t = measure(variants, rounds)
    say("iterations needed %d" % need)
    launches = {}
    for extra in variants:
        variants[extra]()
        launches[extra] = solvers[extra].info()["launches"]          # of the last solve: the enqueue stops at the first look that finds the flag up
        say("max_iter %5d: %10.1f   (last solve: %4d launches enqueued, %4d of them behind the flag)" % (need + extra, t[extra][0], launches[extra], launches[extra] - launches[0]))
    idle = launches[1024] - launches[0]
    say("a live iteration (two launches): %.2f microseconds; launches behind the flag cost %.1f microseconds per solve at max_iter %d%s"
        % (t[0][0] / max(need, 1), t[1024][0] - t[0][0], need + 1024, (" = %.2f each" % ((t[1024][0] - t[0][0]) / idle)) if idle > 0 else ""))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
