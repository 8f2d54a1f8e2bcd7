"""The host side of the operator protocol asks the backend exactly what it was recorded to ask (no GPU): for every case of
tests/operator_protocol_cases.py, each protocol method's ordered backend calls (entry names, shapes / dtypes / strides of tensor
arguments, scalar and keyword values), its hostvals.host_float reads and its exception (type and message) equal the recording in
tests/golden/operator_protocol.json, every tensor it returns equals the recorded one bit for bit, and the capability answers
of the operator equal what the call sites used to derive from its class (tests/golden/make_operator_protocol.py)."""
import json
import os

import numpy as np
import pytest

from tests import operator_protocol_cases as cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def recording():
    with open(os.path.join(GOLD, "operator_protocol.json")) as f:
        gold = json.load(f)
    for case in gold["cases"].values():           # (the file holds every distinct label, backend call and description once)
        case["trace"] = {gold["labels"][label]: dict(gold["values"][value], events=[gold["calls"][i] for i in events])
                         for label, events, value in case["trace"]}
    blob, arrays, at = np.load(os.path.join(GOLD, "operator_protocol.npz"))["bytes"].tobytes(), [], 0
    for dtype, shape in gold["tensors"]:          # (the bytes of the distinct tensors follow each other in this order)
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        arrays.append(np.frombuffer(blob[at:at + n], dtype=dtype).reshape(shape))
        at += n
    return gold["cases"], arrays


def test_every_case_is_recorded(recording):
    assert sorted(recording[0]) == cases.case_names()


@pytest.mark.parametrize("name", cases.case_names())
def test_protocol_trace_and_tensors_match_the_recording(recording, name):
    gold, arrays = recording[0][name], recording[1]
    trace, tensors, _ = cases.run_case(name)
    trace = json.loads(json.dumps(trace))
    for entry in trace.values():
        entry.setdefault("events", [])            # (a call that raises: what it asked before raising is not compared)
    assert sorted(trace) == sorted(gold["trace"])
    for call in sorted(trace):
        assert trace[call] == gold["trace"][call], (name, call)
    assert len(tensors) == len(gold["tensors"])
    for i, (t, key) in enumerate(zip(tensors, gold["tensors"])):
        a, ref = t.contiguous().numpy(), arrays[key]
        assert a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes(), (name, i)


@pytest.mark.parametrize("name", cases.case_names())
def test_capability_answers_match_the_class_expressions(recording, name):
    gold = recording[0][name]["capabilities"]
    _, _, ops = cases.run_case(name)
    assert sorted(ops) == sorted(gold)
    for side, op in ops.items():
        mine = {"kernel_copy_ok": op.kernel_copy_ok,
                "densify_for_wide_solve": [op.densify_for_wide_solve(n) for n in (100, 32768, 32769)],
                "plain_unsharded": op.plain_unsharded,
                "feature_form_kind": op.feature_form_kind}
        assert mine == gold[side], (name, side)
