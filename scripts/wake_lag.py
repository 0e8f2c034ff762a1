"""How late the host wakes behind the last kernel of a replayed headline step, from one rocprofv3 run with
--kernel-trace --hip-trace (no --pmc):

    rocprofv3 --kernel-trace --hip-trace --output-format csv -d OUT -o t -- python3 bench.py --steps 200 --no-extras --no-cpu-baseline
    python scripts/wake_lag.py OUT [STEPS.csv]

For every replayed step (k_bin_count .. k_unit_lean, and k_publish where the build has it), the wake lag is the time from the
end of the step's last kernel to the return of the first host wait (hipEventSynchronize, hipEventQuery, ...) which was in
progress when the kernel ended; the idle time is the step period minus the span from the first kernel start to the last
kernel end.
STEPS.csv, if given, gets one row per step (microseconds from the step's first kernel start)."""
import csv
import glob
import os
import statistics
import sys

SEQ = ["k_bin_count", "k_bin_scatter", "k_bin_sort", "k_brick_query", "k_grid_tail", "k_unit_lean"]
SEQS = (SEQ, SEQ + ["k_publish"])
WAITS = ("hipEventSynchronize", "hipEventQuery", "hipStreamSynchronize", "hipDeviceSynchronize")


def find(d, suffix):
    got = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    if not got:
        sys.exit(f"no *{suffix} under {d}")
    return got[0]


def main(d):
    krows = list(csv.DictReader(open(find(d, "kernel_trace.csv"))))
    krows.sort(key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], []
    for r in krows:
        nm = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("pccm::", "").split("<")[0].strip()
        if nm == "k_bin_count" and cur:
            steps.append(cur)
            cur = []
        cur.append((nm, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    steps.append(cur)
    full = [s for s in steps if [k[0] for k in s] in SEQS]                  # (copies after a step are not part of it)
    full = [s for s in full if len(s) == len(full[-1])]
    full = full[len(full) // 4:]                     # past the eager warm-up, the capture and the first replays

    hrows = [r for r in csv.DictReader(open(find(d, "hip_api_trace.csv"))) if r["Function"] in WAITS]
    waits = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"]) for r in hrows)

    lags, kinds, rows = [], {}, []
    j = 0
    for s in full:
        kend = s[-1][2]
        while j < len(waits) and waits[j][1] < kend:
            j += 1
        k = j                                           # the first wait still in progress when the kernel ended
        if k < len(waits) and waits[k][0] <= kend:
            lags.append((waits[k][1] - kend) / 1e3)
            kinds[waits[k][2]] = kinds.get(waits[k][2], 0) + 1
        rows.append([(x - s[0][1]) / 1e3 for x in (s[-1][1], kend)] + [lags[-1] if k < len(waits) and waits[k][0] <= kend else ""])
    span = [(s[-1][2] - s[0][1]) / 1e3 for s in full]
    period = [(b[0][1] - a[0][1]) / 1e3 for a, b in zip(full, full[1:])]
    idle = [p - sp for p, sp in zip(period, span)]
    q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]
    print(f"{len(full)} replayed steps; {len(lags)} with a host wait in progress at the end of {full[0][-1][0]} ({kinds})")
    for i, k in enumerate(full[0]):
        print(f"  {k[0]:16s} {statistics.median(s[i][2] - s[i][1] for s in full) / 1e3:6.1f} us")
    print(f"  kernels first start -> last end  median {statistics.median(span):6.1f} us")
    print(f"  step period                      median {statistics.median(period):6.1f} us")
    print(f"  GPU idle between steps           median {statistics.median(idle):6.1f} us  p10 {q(idle, .1):6.1f}  p90 {q(idle, .9):6.1f}")
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write("step,last_kernel_start_us,last_kernel_end_us,wait_return_after_end_us,next_step_start_us\n")
            for i, r in enumerate(rows):
                nxt = f"{(full[i + 1][0][1] - full[i][0][1]) / 1e3:.1f}" if i + 1 < len(full) else ""
                lag = f"{r[2]:.1f}" if r[2] != "" else ""
                f.write(f"{i},{r[0]:.1f},{r[1]:.1f},{lag},{nxt}\n")
    if lags:
        print(f"  last kernel end -> wait returns  median {statistics.median(lags):6.1f} us  p10 {q(lags, .1):6.1f}  p90 {q(lags, .9):6.1f}")


if __name__ == "__main__":
    main(sys.argv[1])
