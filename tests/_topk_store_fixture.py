"""Integer-factor ALS store shared by the top-N tests (CPU and GPU).

Rank 4, every factor a small integer (exact in bf16).  A live item's vector
is the base-4 digits of a number ``m`` of its own and a user's vector is a
permutation of (64, 16, 4, 1), so every user sees pairwise distinct item
scores -- except items 12 and 31, which share ``m`` on purpose (one lives in
the bulk blocks, one in the row mirror) to pin the cross-source tie order.
Superseded values are [3, 3, 3, 3] (m = 255, the best possible score for
every user) and MEAN-I is [9, 9, 9, 9]: either would top every list if it
leaked into the candidates.
"""

import torch

from flink_ms_amd.serving import ALSModelStore

USERS = {"1": (64, 16, 4, 1), "2": (1, 4, 16, 64), "3": (16, 64, 1, 4),
         "4": (4, 1, 64, 16), "5": (64, 4, 16, 1)}
# live items: id -> m
BULK = {10: 7, 11: 201, 12: 99, 13: 250, 14: 3, 15: 64, 16: 129, 17: 30,
        18: 177, 19: 58}
ATTACH = {20: 254, 21: 11, 22: 85, 23: 170, 24: 42, 25: 200, 26: 1, 27: 131}
ROWS = {30: 233, 31: 99, 32: 16, 33: 78, 11: 120}   # 11 shadows the bulk row
LIVE = {**{str(i): m for i, m in BULK.items()},
        **{str(i): m for i, m in ATTACH.items()},
        **{str(i): m for i, m in ROWS.items()}}


def digits(m):
    return [float(m // 64 % 4), float(m // 16 % 4), float(m // 4 % 4),
            float(m % 4)]


def _row(eid, kind, vec):
    return f"{eid},{kind}," + ";".join(repr(float(x)) for x in vec)


def build_store(device) -> ALSModelStore:
    store = ALSModelStore(device=device)
    # bulk block: users 1, 2; items 10..19, item 10 first with a stale value
    stale = [_row(10, "I", digits(255))]
    block = ([_row(u, "U", USERS[u]) for u in ("1", "2")] + stale
             + [_row(i, "I", digits(m)) for i, m in BULK.items() if i != 10])
    store.ingest_bulk("\n".join(block) + "\n")
    store.ingest_bulk(_row(10, "I", digits(BULK[10])) + "\n")   # new slot
    # attach: users 3, 4; items 20..27, then item 20 attached again
    uf = torch.tensor([USERS["3"], USERS["4"]], dtype=torch.float32)
    ids = sorted(ATTACH)
    store.attach_factors(
        uf, torch.tensor([digits(255 if i == 20 else ATTACH[i])
                          for i in ids]),
        user_ids=torch.tensor([3, 4]), item_ids=torch.tensor(ids))
    store.attach_factors(
        torch.tensor([USERS["4"]], dtype=torch.float32),
        torch.tensor([digits(ATTACH[20])]),
        user_ids=torch.tensor([4]), item_ids=torch.tensor([20]))
    # row at a time: user 5, items 30..33, the MEAN rows, and item 11 again
    store.ingest_row(_row(5, "U", USERS["5"]))
    store.ingest_row(_row("MEAN", "I", [9.0] * 4))
    store.ingest_row(_row("MEAN", "U", [9.0] * 4))
    for i, m in ROWS.items():
        store.ingest_row(_row(i, "I", digits(m)))
    return store


def brute_force(store, user, n, exclude=()):
    """fp64 ranking over get_vector: score descending, then numeric id."""
    u = store.get_vector(f"{user}-U")
    ranked = []
    for item in LIVE:
        if item in exclude:
            continue
        v = store.get_vector(f"{item}-I")
        ranked.append((-sum(a * b for a, b in zip(u, v)), int(item)))
    ranked.sort()
    return ([str(i) for _, i in ranked[:n]], [-s for s, _ in ranked[:n]])
