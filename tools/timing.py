"""The timing method of the PNG tools (tools/png*time.py), and so of the PNG figures in DESIGN.md: device events around
`calls` back-to-back calls, two warm-up calls per variant, then `rounds` rounds in which the variants ALTERNATE, so that
drift of the machine falls on all of them alike.  A round times as many calls as fill a window of half a second, or a
fixed number where the tool says so.  Per variant: median, minimum and maximum over the rounds -- the spread is what a
difference between two variants must exceed.

A tool run as `python tools/X.py` has its own directory on sys.path: `import timing`.
"""
import math
import sys

import torch

SHOW = "%-52s median %9.3f ms, min %9.3f, max %9.3f over %d rounds of %d calls, %.0f GB/s"


def once(f, calls):
    """Milliseconds per call over `calls` calls on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def interleaved(variants, rounds, window_ms=500.0, calls=None):
    """variants: ((name, f), ..) -> ({name: [ms per call, one per round]}, {name: calls per round})."""
    per_round = {}
    for name, f in variants:
        f()
        f()
        torch.cuda.synchronize()
        per_round[name] = calls if calls is not None else max(1, int(math.ceil(window_ms / max(once(f, 1), 1e-3))))
    ts = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, f in variants:
            ts[name].append(once(f, per_round[name]))
    return ts, per_round


def show(name, t, calls, nbytes, fmt=SHOW):
    """Prints median, minimum, maximum and GB/s of one variant (fmt: the tool's own columns) -> the median."""
    t = sorted(t)
    med = t[len(t) // 2]
    print(fmt % (name, med, t[0], t[-1], len(t), calls, nbytes / med / 1e6))
    return med


def measure(variants, rounds, width=62):
    """Times the variants and prints each one -> [(median, minimum, maximum)] in their order."""
    ts, calls = interleaved(variants, rounds)
    stats = []
    for name, _ in variants:
        t = sorted(ts[name])
        stats.append((t[len(t) // 2], t[0], t[-1]))
        print("  %-*s median %9.3f ms [%9.3f .. %9.3f] over %d rounds of %d calls" % (width, name, t[len(t) // 2], t[0], t[-1], len(t), calls[name]))
    return stats


def compare(title, variants, rounds):
    """Prints every variant; the first is the mixed call, the second what it is held against: it may take the second's
    median plus both spreads plus 5 %."""
    stats = measure(variants, rounds)
    (m, mlo, mhi), (p, plo, phi) = stats[0], stats[1]
    allowed = p + (phi - plo) + (mhi - mlo) + 0.05 * p
    print("  %s: mixed / per-geometry = %.3f; allowance (spreads + 5 %%) %.3f ms: %s by %.3f ms" %
          (title, m / p, allowed, "inside" if m <= allowed else "MISSED", abs(allowed - m)))
    sys.stdout.flush()
    return stats


def arange_off(n, step, start=0, device="cuda"):
    """Offsets of n slots of `step` bytes from byte `start`."""
    return start + torch.arange(n + 1, dtype=torch.int64, device=device) * step
