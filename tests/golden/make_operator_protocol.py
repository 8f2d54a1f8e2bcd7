"""Generates tests/golden/operator_protocol.json and operator_protocol.npz from THIS project's own operators (no reference
code involved): for every case of tests/operator_protocol_cases.py, what each protocol method asks of the backend and what it
returns, and the capability answers the call sites used to derive from the operator's class.

Run from the repository root, on the commit whose behaviour is to be kept:
    python -B tests/golden/make_operator_protocol.py

The json holds every distinct label, backend call and result description once and, per case and protocol call, their
indices; every distinct returned tensor is stored once, its dtype and shape in the json and its bytes in the npz.
"""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
sys.dont_write_bytecode = True


def class_capabilities(op):
    """The capability answers as the call sites wrote them before the operators answered for themselves: by class identity."""
    from rpgp_amd.operators import AdditiveRPOperator, FamilyAdditiveOperator, SKIAdditiveOperator
    plain = type(op) is AdditiveRPOperator
    weighted = type(op) is FamilyAdditiveOperator and op.kind == "RBF" and op.group == 1 and not op.product
    return {
        "kernel_copy_ok": isinstance(op, AdditiveRPOperator) and not isinstance(op, SKIAdditiveOperator) and
        op.Z1.dtype == torch.float32 and getattr(op, "cacheable", True),
        "densify_for_wide_solve": [not (isinstance(op, SKIAdditiveOperator) and n > 32768) for n in (100, 32768, 32769)],
        "plain_unsharded": plain and (op.shard is None or op.shard.world_size <= 1),
        "feature_form_kind": None if not op.symmetric else "plain" if plain else "weighted" if weighted else None,
    }


def main():
    import rpgp_amd  # noqa: F401
    from tests import operator_protocol_cases as cases
    traces, arrays, calls, values, labels = {}, {}, {}, {}, {}

    def intern(table, value):
        return table.setdefault(json.dumps(value, sort_keys=True), len(table))
    for name in cases.case_names():
        trace, tensors, ops = cases.run_case(name)
        keys = []
        for t in tensors:
            a = t.contiguous().numpy()
            keys.append(list(arrays.setdefault((str(a.dtype), a.shape, a.tobytes()), (len(arrays), a)))[0])
        # per protocol call: [label, what it asked the backend, the rest of its entry], as indices into the three tables
        packed = [[intern(labels, label), [intern(calls, e) for e in entry.pop("events", [])], intern(values, entry)]
                  for label, entry in trace.items()]
        traces[name] = {"trace": packed, "tensors": keys,
                        "capabilities": {side: class_capabilities(op) for side, op in ops.items()}}
    stored = [a for _, a in arrays.values()]
    tables = {"labels": labels, "calls": calls, "values": values}
    with open(os.path.join(OUT, "operator_protocol.json"), "w") as f:
        f.write("{")
        for key, table in tables.items():
            f.write('"%s": %s,\n ' % (key, json.dumps([json.loads(e) for e in table], sort_keys=True, separators=(",", ":"))))
        f.write('"tensors": %s,\n ' % json.dumps([[str(a.dtype), list(a.shape)] for a in stored], separators=(",", ":")))
        f.write('"cases": {\n' + ",\n".join('  "%s": %s' % (name, json.dumps(traces[name], sort_keys=True, separators=(",", ":")))
                                            for name in sorted(traces)) + "\n }}\n")
    # the bytes of the distinct tensors, one after the other in the order of "tensors"
    blob = np.frombuffer(b"".join(a.tobytes() for a in stored), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "operator_protocol.npz"), bytes=blob)
    print("%d cases, %d tensors written to %s" % (len(traces), len(stored), OUT))


if __name__ == "__main__":
    main()
