"""What HjbNativePlan decides for the configurations of tests/hjb_plan_cases.py, against a recorded table.

tests/golden/hjb_plan_decisions.json holds `observe(plan)` of every case (or the constructor's refusal) as the plan answered on a
256-CU device when the table was recorded: state basis, matrix mode, range guard, store_path, kernel instance, chunking, hipGraph
replay, the u_L2 log's form and the scratch sizes.  A host refactor of plan_native.py must leave it as it is.  A deliberate change
of a selection rule re-records it, on the GPU:

    python tests/test_gpu_hjb_plan_table.py --record
"""
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN_DIR
from hjb_plan_cases import CASES, NAMES, build_solver, observe, outcome
from util_cases import psp

GOLDEN = os.path.join(GOLDEN_DIR, "hjb_plan_decisions.json")
SWITCHES = ("PSP_STATE_BASIS", "PSP_FORCE_WIDE", "PSP_FWD_COOP", "PSP_FWD_VARIANT")


def row(case, device):
    def build():
        model = build_solver(case, device)
        return observe(psp.plan_native.HjbNativePlan(model, noise=model.noise))
    return outcome(build)


def record():
    for name in SWITCHES:
        os.environ.pop(name, None)
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = ",\n".join('%s:%s' % (json.dumps(c["name"]), json.dumps(row(c, dev), sort_keys=True, separators=(",", ":"))) for c in CASES)
    with open(GOLDEN, "w") as fh:
        fh.write('{"cus":%d,\n"rows":{\n%s\n}}\n' % (cus, rows))
    print("%d rows on %d CUs, %d bytes" % (len(CASES), cus, os.path.getsize(GOLDEN)))


def load_table():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.gpu
def test_plans_decide_as_recorded(monkeypatch):
    gold = load_table()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if cus != gold["cus"]:
        pytest.skip("the table was recorded on %d CUs; this device has %d" % (gold["cus"], cus))
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert list(gold["rows"]) == NAMES, "hjb_plan_cases.CASES is no longer the list the table was recorded on"
    wrong = []
    for case in CASES:
        got, want = row(case, dev), gold["rows"][case["name"]]
        if got != want:
            wrong.append((case["name"], {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}))
    assert not wrong, "%d of %d rows differ (row, {field: (plan, recorded)}): %r" % (len(wrong), len(CASES), wrong[:5])


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
