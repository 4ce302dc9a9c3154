"""The A/B gate of the kernel benchmarks (kbench.py, lnbench.py): alternated timings of an old and a new form in one process.

The new form passes when its median lies below the old median by more than the old form's interquartile range, over at least 15
alternated rounds.  (The gate used to compare against the old form's min-to-max spread: a single outlier among the old timings then
decided - QKV on the 384-row tile failed it on one 1.653 ms sample beside a 1.307 ms median, profiles/gemm384.txt 3.)
Quartiles are order statistics of the sorted timings, no interpolation: q1 = t[n // 4], median = t[n // 2], q3 = t[(3 * n) // 4].
"""

MIN_ROUNDS = 15


def quartiles(times):
    t = sorted(times)
    n = len(t)
    return t[n // 4], t[n // 2], t[(3 * n) // 4]


def gate(old_times, new_times):
    """-> (passed, text).  passed is None when there are too few rounds to decide."""
    q1, med_old, q3 = quartiles(old_times)
    med_new = quartiles(new_times)[1]
    gain, iqr = med_old - med_new, q3 - q1
    text = f"old median {med_old:.4f} IQR {iqr:.4f} ({q1:.4f}..{q3:.4f})  new median {med_new:.4f}  gain {gain:+.4f} ({gain / med_old * 100:+.2f} %)"
    if min(len(old_times), len(new_times)) < MIN_ROUNDS:
        return None, text + f"  gate: undecided (needs >= {MIN_ROUNDS} rounds)"
    return gain > iqr, text + ("  gate: PASSED" if gain > iqr else "  gate: not passed")
