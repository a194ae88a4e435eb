"""The plan handle's dispatch: one small plan of every kind and precision, built and never executed (tools/plan_handle_table.py),
answers every field of fft_gpu_plan_info_hip, every getter, every option, the team status and the refusal of fft_gpu_execute_ptr_hip
exactly as tests/golden/plan_handle_table.json records it -- the table the same tool printed on an MI355X before the handle's 24 typed
pointers became one set per precision.  A plan kind that a list of the handle forgets (its cores, an option, a getter, its fill)
shows here as a changed field."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("plan_handle_table", os.path.join(ROOT, "tools", "plan_handle_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_equals_the_recorded_one(gpu_lib):
    with open(os.path.join(ROOT, "tests", "golden", "plan_handle_table.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(load_tool().build_table()))  # (through JSON: lists and string keys on both sides)
    assert sorted(got["plans"]) == sorted(want["plans"])
    for name, row in want["plans"].items():
        have = row.keys() | got["plans"][name].keys()
        for section in sorted(have):
            w, g = row.get(section), got["plans"][name].get(section)
            if isinstance(w, dict) and isinstance(g, dict):
                for field in sorted(w.keys() | g.keys()):
                    assert g.get(field) == w.get(field), "%s: %s.%s is %r, recorded %r" % (name, section, field, g.get(field), w.get(field))
            else:
                assert g == w, "%s: %s is %r, recorded %r" % (name, section, g, w)
    # every plan was destroyed; each one made exactly one stream
    assert got["streams_created"] == want["streams_created"] == len(want["plans"])
