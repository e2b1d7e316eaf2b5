"""profiles/dense_bwd_errors.txt from the printed output of tests/test_dense_bwd_gpu.py (pytest -s): per shape, row count and output the
largest error of either path over the runs and the largest share of the bound a run used.
    python scripts/summarize_dense_bwd_errors.py PYTEST_OUTPUT > profiles/dense_bwd_errors.txt"""
import collections
import re
import sys

PAT = re.compile(r"DENSEBWD (\d+x\d+) R=(\d+) G=(\d) bias=(\d) (\w+) (dX|dW|db): pair err (\S+) fused err (\S+) ratio (\S+) bound (\S+) max\|ref\| (\S+)")


def main(path):
    lines = [l[l.index("DENSEBWD"):] for l in open(path) if "DENSEBWD" in l]
    agg = collections.OrderedDict()
    for l in lines:
        m = PAT.match(l)
        if not m:
            continue
        shp, R, _, _, _, out, eo, en, _, bound, sc = m.groups()
        eo, en, bound, sc = float(eo), float(en), float(bound), float(sc)
        a = agg.setdefault((shp, int(R), out), dict(eo=0.0, en=0.0, use=0.0, n=0, sc=sc))
        a["eo"], a["en"], a["n"] = max(a["eo"], eo), max(a["en"], en), a["n"] + 1
        a["use"] = max(a["use"], en / bound if bound > 0 else 0.0)
    print("magpo_dense_bwd against fp64, next to the pair magpo_wgrad + magpo_linear on the same inputs (tests/test_dense_bwd_gpu.py, MI355X).\n"
          "Per shape, row count and output: the largest error of either path over G in {1, 4}, bias on / off and the three mask modes (12 runs,\n"
          "6 for db), and the largest fraction of the bound  2 x pair error + 1e-7 x max|reference|  that the fused kernel used in any one run.\n"
          "The kernel sums the pair's terms in the pair's order, so the two columns agree (test_same_values_as_the_pair: equal element for element).\n")
    print(f"{'shape':8} {'R':>6} {'out':3} {'runs':>4} {'pair max err':>12} {'fused max err':>13} {'ratio':>6} {'max err/bound':>13} {'max|ref|':>10}")
    for (shp, R, out), a in agg.items():
        print(f"{shp:8} {R:6d} {out:3} {a['n']:4d} {a['eo']:12.3e} {a['en']:13.3e} {a['en'] / max(a['eo'], 1e-300):6.2f} {a['use']:13.2f} {a['sc']:10.3e}")
    print("\nGuider / actor level (one minibatch, threshold 0 against the default):")
    for l in lines:
        if l.startswith("DENSEBWD learner"):
            print(l[9:], end="")


if __name__ == "__main__":
    main(sys.argv[1])
