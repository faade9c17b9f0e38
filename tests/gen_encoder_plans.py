"""Dump the encoder's host-side plans as JSON: the record tests/test_encoder_state_host.py holds the Python host to
(tests/golden/encoder_plans_parent.json).

For every config below, with and without the pooling head: the parameter table as (label, ABI field, shape) in order,
the weight-shadow unit of every entry, the gradient chunk layout for max_buckets in {1, 2, 8, 64} under every pattern of
``needs_patterns``, and the hidden-state slot plan for five tap sets (reduced modulo L + 1, distinct and ascending, as
``forward`` hands them to the op) with train on and off.  Two layouts (everything
trainable; frozen below block 1) are stored in full at 2 and 8 buckets, everything else as the SHA-256 of its canonical
JSON; the two full-size configs (built on the meta device: the plans need shapes only) are stored as digests throughout.

The committed file was written by the commit BEFORE encoder.py was split into surfaces / ops / state owners.  To
regenerate it, copy this file into a checkout of that commit and run it there with ``--parent``, which selects the
spellings of that commit:

    parent (``--parent``)                                   now
    ------------------------------------------------------  ---------------------------------------------------
    zip(m._flat_names, m._flat_params())                    m._table.entries (label, field) + m._table.params()
    int(label[5:]) for "layerN" labels, else L              entry.unit
    m._bucket_layout(needs)                                 m._grads.layout(needs)
    pkg.encoder._slot_plan                                  pkg.encoder_ops._slot_plan

``m.set_grad_reducer(GradBucketReducer(max_buckets=n))`` selects the chunk count in both.  Needs no GPU.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "encoder_plans_parent.json")

SMALL = ["tiny", "hostile"]                                   # full lists for FULL_LAYOUTS, digests for the rest
LARGE = ["so400m-patch14-384", "base-patch16-224"]            # meta device, digests only
MAX_BUCKETS = [1, 2, 8, 64]
FULL_LAYOUTS = [f"{pat}@{mb}" for pat in ("all", "frozen_below_1") for mb in (2, 8)]


class Current:
    @staticmethod
    def table(m):
        return [(e.label, e.field, tuple(p.shape)) for e, p in zip(m._table.entries, m._table.params())]

    @staticmethod
    def units(m):
        return [e.unit for e in m._table.entries]

    @staticmethod
    def layout(m, needs):
        return m._grads.layout(needs)

    @staticmethod
    def slot_plan(pkg):
        return pkg.encoder_ops._slot_plan


class Parent:
    @staticmethod
    def table(m):
        return [(grp, field, tuple(p.shape)) for (grp, field), p in zip(m._flat_names, m._flat_params())]

    @staticmethod
    def units(m):
        L = m.config.num_hidden_layers
        return [int(grp[5:]) if grp.startswith("layer") else L for grp, _ in m._flat_names]

    @staticmethod
    def layout(m, needs):
        return m._bucket_layout(needs)

    @staticmethod
    def slot_plan(pkg):
        return pkg.encoder._slot_plan


def canonical(obj) -> str:
    return json.dumps(obj, sort_keys=True, separators=(",", ":"))


def digest(obj) -> str:
    return hashlib.sha256(canonical(obj).encode()).hexdigest()


def dumps(t) -> str:
    """The record as JSON with one line per table, unit list, layout and slot plan, so that a diff names what moved."""
    def lines(d, depth):
        if depth == 0:
            return canonical(d)
        pad = " " * (3 - depth)
        return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {lines(d[k], depth - 1 if isinstance(d[k], dict) else 0)}"
                                  for k in sorted(d)) + "\n" + pad[1:] + "}"
    return lines(t, 3) + "\n"


def needs_patterns(table, L):
    """{name: [bool per table entry]}.  A block's number is its position among the labels: the table lists the
    embeddings, block 0 .. L-1, then the post-LN and head."""
    labels = list(dict.fromkeys(lbl for lbl, _, _ in table))
    assert len(labels) == L + 2 and labels[0] == "emb" and labels[-1] == "head"
    block = {lbl: i - 1 for i, lbl in enumerate(labels) if 0 < i <= L}
    pats = {"all": [True] * len(table), "none": [False] * len(table),
            "head_only": [lbl == "head" for lbl, _, _ in table], "emb_only": [lbl == "emb" for lbl, _, _ in table]}
    for k in range(1, L + 1):
        pats[f"frozen_below_{k}"] = [lbl == "head" or block.get(lbl, -1) >= k for lbl, _, _ in table]
    for lbl, field, _ in table:
        if block.get(lbl) == 1:
            pats[f"block1_{field}_frozen"] = [(l2, f2) != (lbl, field) for l2, f2, _ in table]
    pats["only_block0_q_w"] = [block.get(lbl) == 0 and field == "q_w" for lbl, field, _ in table]
    return pats


def tap_sets(L):
    return {"none": (), "first": (0,), "last": (L,), "1_3": (1, 3), "all": tuple(range(L + 1))}


def record(pkg, api, name, use_head, full):
    """The plans of one model.  ``full``: keep the table, the units and FULL_LAYOUTS as lists."""
    cfg = dataclasses.replace(pkg.get_config(name), vision_use_head=use_head)
    L = cfg.num_hidden_layers
    with torch.device("meta"):
        m = pkg.SiglipVisionModelHIP(cfg, compute_dtype="fp32")
    table, units = api.table(m), api.units(m)
    layouts = {}
    for mb in MAX_BUCKETS:
        m.set_grad_reducer(pkg.GradBucketReducer(max_buckets=mb))
        for pat, needs in needs_patterns(table, L).items():
            key = f"{pat}@{mb}"
            chunks, groups = api.layout(m, needs)
            plan = json.loads(canonical({"chunks": chunks, "groups": groups}))
            layouts[key] = plan if full and key in FULL_LAYOUTS else digest(plan)
    slot_plan = api.slot_plan(pkg)
    slots = {f"{tag}/{int(train)}": digest(json.loads(canonical(slot_plan(sorted({t % (L + 1) for t in taps}), train, L))))
             for tag, taps in tap_sets(L).items() for train in (False, True)}
    as_lists = json.loads(canonical({"table": table, "units": units}))
    return {"table": as_lists["table"] if full else digest(as_lists["table"]),
            "units": as_lists["units"] if full else digest(as_lists["units"]), "layouts": layouts, "slots": slots}


def sweep(pkg, api=Current):
    return {f"{name}/{'head' if use_head else 'nohead'}": record(pkg, api, name, use_head, name in SMALL)
            for name in SMALL + LARGE for use_head in (True, False)}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    t = sweep(pkg, Parent if "--parent" in sys.argv[1:] else Current)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(dumps(t))
    print(f"wrote {OUT}: {len(t)} models, {os.path.getsize(OUT)} bytes")
