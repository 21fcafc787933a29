"""The census of kernel forms (tools/form_census.py) against the recorded one, tests/golden/form_census.json: for every configuration
-- the smallest shapes of the suite at which a form decision of sg_forward / sp_detect flips -- the ordered (name, form, launches) rows
of the timing report and the CRC32 of every output tensor's bytes must be the recorded ones.  The kernels are deterministic and the
suite already relies on run-to-run bit identity, so the tolerance is equality.  The file was recorded before plan_superglue /
plan_superpoint replaced the decisions spread over the launch loops: a planner that picks another form, another order or other
arguments anywhere fails here.  Several forms are chosen by the CU count, so a device with another count than the recorded one
skips.  Needs an MI355X."""
import importlib.util
import json
import os

import pytest

from tests import util

_spec = importlib.util.spec_from_file_location("form_census", os.path.join(os.path.dirname(util.GOLDEN), os.pardir, "tools", "form_census.py"))
form_census = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(form_census)

pytestmark = pytest.mark.gpu

with open(os.path.join(util.GOLDEN, "form_census.json")) as fh:
    RECORDED = json.load(fh)


def test_the_recorded_census_covers_every_configuration():
    assert sorted(RECORDED["configs"]) == sorted(form_census.CONFIGS)


@pytest.mark.parametrize("name", list(form_census.CONFIGS))
def test_forms_and_output_bytes_equal_the_recorded_census(name):
    if form_census.cu_count() != RECORDED["cu_count"]:
        pytest.skip(f"the census was recorded on a device with {RECORDED['cu_count']} CUs, this one has {form_census.cu_count()}")
    got, want = form_census.run(name), RECORDED["configs"][name]
    assert got["rows"] == want["rows"], f"{name}: the launches differ from the recorded ones\n got  {got['rows']}\n want {want['rows']}"
    assert got["crc32"] == want["crc32"], f"{name}: output bytes differ from the recorded run: {got['crc32']} vs {want['crc32']}"
