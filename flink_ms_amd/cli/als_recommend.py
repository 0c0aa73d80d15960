"""Interactive ALS recommendation client (no reference analog; the shape of
ALSPredict.java's REPL).

Usage: ``als_recommend <jobID> [<jobManagerHost>] [<jobManagerPort>]`` — jobID
is accepted for CLI parity (the HTTP server needs no job id).  Reads
``user[,n]`` lines (n defaults to 10), asks /als/recommend for the user's
top-n items and prints one ``item<TAB>score`` row per item.
"""
import sys

from ..serving.client import QueryClientHelper


def main(argv=None) -> int:
    args = sys.argv[1:] if argv is None else argv
    if not args:
        print("Missing required job ID argument. "
              "Usage: ./ALSRecommend <jobID> [jobManagerHost] "
              "[jobManagerPort]")
        return 1
    host = args[1] if len(args) > 1 else "localhost"
    port = int(args[2]) if len(args) > 2 else 6123
    print(f"Using JobManager {host}:{port}")
    print("Enter <User[,N]> to recommend.")
    with QueryClientHelper(host, port) as client:
        for line in sys.stdin:
            key = line.upper().strip()
            if not key:
                continue
            print(f"[info] Querying the model for user '{key}'")
            try:
                user_id, _, count = key.partition(",")
                n = int(count) if count.strip() else 10
                res = client.als_recommend([user_id.strip()], n)
                if res["found"][0]:
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
