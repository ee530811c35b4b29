"""The insert span per scan from a rocprofv3 kernel trace: first k_ins_prep
start to k_push_window end, and each insert kernel's median duration.

    python scripts/insert_span.py <trace dir>/run_kernel_trace.csv [scans_from_end]
"""
import csv
import sys

from scan_timeline import short


def main():
    path = sys.argv[1]
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]))
                  for r in csv.DictReader(open(path)))
    spans, per, t0 = [], {}, None
    for s, e, n in rows:
        base = n.split("<")[0]
        if base == "k_ins_prep":
            t0 = s
            cur = {}
        if t0 is None or not (base.startswith("k_ins_") or base in ("k_seg_offsets", "k_push_window")):
            continue
        cur[base] = (e - s) / 1e3
        if base == "k_push_window":
            spans.append(((e - t0) / 1e3, cur))
            t0 = None
    spans = spans[-back:]
    med = lambda v: sorted(v)[len(v) // 2]
    print("insert span us (last %d scans): median %.1f  min %.1f  max %.1f" %
          (len(spans), med([x for x, _ in spans]), min(x for x, _ in spans), max(x for x, _ in spans)))
    for k in spans[-1][1]:
        print("  %-20s median %.1f us" % (k, med([c[k] for _, c in spans if k in c])))


if __name__ == "__main__":
    main()
