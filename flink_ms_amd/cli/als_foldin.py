"""Interactive ALS fold-in client (no reference analog; the shape of
ALSPredict.java's REPL).

Usage: ``als_foldin <jobID> [<jobManagerHost>] [<jobManagerPort>] --lambda L
[--implicitPrefs true] [--alpha A] [--n N]`` — jobID is accepted for CLI
parity (the HTTP server needs no job id); ``--lambda`` is the training
regularization.  Reads one basket per line, ``item[:value],item[:value],...``
(a missing value means 1), asks /als/foldin for the new user's top-n items
(n defaults to 10) and prints one ``item<TAB>score`` row per item.
"""
import sys

from ..serving.client import QueryClientHelper

USAGE = ("Usage: ./ALSFoldIn <jobID> [jobManagerHost] [jobManagerPort] "
         "--lambda L [--implicitPrefs true] [--alpha A] [--n N]")


def main(argv=None) -> int:
    args = list(sys.argv[1:] if argv is None else argv)
    flags = {}
    pos = []
    while args:
        a = args.pop(0)
        if a.startswith("--"):
            if not args:
                print(f"Missing value for {a}. {USAGE}")
                return 1
            flags[a[2:]] = args.pop(0)
        else:
            pos.append(a)
    if not pos:
        print(f"Missing required job ID argument. {USAGE}")
        return 1
    if "lambda" not in flags:
        print(f"Missing required --lambda argument. {USAGE}")
        return 1
    unknown = set(flags) - {"lambda", "implicitPrefs", "alpha", "n"}
    if unknown:
        print(f"Unknown argument --{sorted(unknown)[0]}. {USAGE}")
        return 1
    reg = float(flags["lambda"])
    implicit = flags.get("implicitPrefs", "false").strip().lower() == "true"
    alpha = float(flags.get("alpha", 1.0))
    n = int(flags.get("n", 10))
    host = pos[1] if len(pos) > 1 else "localhost"
    port = int(pos[2]) if len(pos) > 2 else 6123
    print(f"Using JobManager {host}:{port}")
    print("Enter <Item[:Value],Item[:Value],...> to fold in.")
    with QueryClientHelper(host, port) as client:
        for line in sys.stdin:
            key = line.upper().strip()
            if not key:
                continue
            print(f"[info] Querying the model for basket '{key}'")
            try:
                items, values = [], []
                for tok in key.split(","):
                    if not tok.strip():
                        continue
                    item, _, value = tok.partition(":")
                    items.append(item.strip())
                    values.append(float(value) if value.strip() else 1.0)
                res = client.als_fold_in([items], [values],
                                         regularization=reg,
                                         implicit=implicit, alpha=alpha, n=n)
                if res["used"][0]:
                    for item, score in zip(res["items"][0],
                                           res["scores"][0]):
                        print(f"{item}\t{score:f}")
                else:
                    print("User or Item Factors do not exist in the model "
                          f"for the query: {key}")
            except Exception as e:  # noqa: BLE001
                print("Query failed because of the following Exception:")
                print(e)
    return 0


if __name__ == "__main__":
    sys.exit(main())
