"""ALS training job (reference flink-als/.../ALSImpl.scala rebuild).

Flags (ALSImpl.scala:22-62): --input, --fieldDelimiter (comma|tab, comma),
--ignoreFirstLine (true), --iterations (10), --numFactors (10), --blocks,
--temporaryPath, --lambda (0.9), --seed (42), --itemFactors, --userFactors.
``--implicitPrefs`` (false) and ``--alpha`` (1.0) select confidence-weighted
ALS for implicit feedback (Spark's flags of the same names): the rating
column is an interaction strength, confidence 1 + alpha*|r|, preference
[r > 0].  The model files keep their format.
``--blocks`` is accepted for CLI parity (blocking is GPU-count-driven).
``--temporaryPath <dir>`` stages each iteration's factors to disk in the
model text format — the reference uses the flag to trade memory
(ALSImpl.scala:42-44 [EXT]); with 288 GB HBM/GPU the memory trade is
unnecessary, so here it buys restartable/inspectable training instead
(re-launch with the staged files as a warm start via the model formats).
"""

from __future__ import annotations

import os
import sys

import torch

from ..data.ratings import load_ratings_csv
from ..models.als import ALSConfig, ALSTrainer
from ..parallel.dist import init_from_env
from ..utils.params import Params


def main(argv=None) -> int:
    params = Params.from_args(sys.argv[1:] if argv is None else argv)
    if not params.has("input"):
        print("Use --input to specify file input.")
        return 0
    ctx = init_from_env()
    users, items, ratings = load_ratings_csv(
        params.get_required("input"),
        field_delimiter=params.get("fieldDelimiter", "comma"),
        ignore_first_line=params.get_bool("ignoreFirstLine", True),
    )
    num_users = int(users.max()) + 1
    num_items = int(items.max()) + 1
    cfg = ALSConfig(
        iterations=params.get_int("iterations", 10),
        num_factors=params.get_int("numFactors", 10),
        lambda_=params.get_float("lambda", 0.9),
        seed=params.get_int("seed", 42),
        implicit_prefs=params.get_bool("implicitPrefs", False),
        alpha=params.get_float("alpha", 1.0),
        dtype=torch.bfloat16 if ctx.device.type == "cuda" else torch.float32,
    )
    trainer = ALSTrainer(cfg, ctx)
    trainer.setup(users.long(), items.long(), ratings, num_users, num_items)
    tmp = params.get("temporaryPath")
    for it in range(cfg.iterations):
        trainer.step()
        if tmp:
            d = os.path.join(tmp, f"iteration-{it}")
            os.makedirs(d, exist_ok=True)
            snap = trainer.model()
            part = f"part-{ctx.rank}" if ctx.world_size > 1 else ""
            with open(os.path.join(d, f"userFactors{part}"), "w") as uf_f, \
                    open(os.path.join(d, f"itemFactors{part}"), "w") as if_f:
                snap.write(uf_f, if_f)
    model = trainer.model()
    if params.has("itemFactors") and params.has("userFactors"):
        upath = params.get("userFactors")
        ipath = params.get("itemFactors")
        if ctx.world_size > 1:  # one part file per rank (writeAsText dirs)
            os.makedirs(upath, exist_ok=True)
            os.makedirs(ipath, exist_ok=True)
            upath = os.path.join(upath, f"part-{ctx.rank}")
            ipath = os.path.join(ipath, f"part-{ctx.rank}")
        with open(upath, "w") as uf, open(ipath, "w") as itf:
            model.write(uf, itf)
        print(f"[ALS] model-training done: {trainer.timings.mean_iter:.3f}"
              " s/iteration")
    else:
        print("Printing results to stdout. Use --itemFactors and "
              "--userFactors to specify output locations.")
        import io
        uf, itf = io.StringIO(), io.StringIO()
        model.write(uf, itf)
        print("==== USER FACTORS ====")
        print(uf.getvalue(), end="")
        print("==== ITEM FACTORS ====")
        print(itf.getvalue(), end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
