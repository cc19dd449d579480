"""CPU: the host-side plan of `event` against a recorded table, row for row.

tests/golden/event_plan_table.npz holds what the library answered -- sgk_event_plan_opt's nine fields and the three
workspace sizes (sgk_event_workspace_bytes_opt; sgk_event_workspace_bytes_param for a generic-route set and for the
presets' kernels) -- for 15 600 batches: 15 read counts x 13 mean lengths x 5 ratios of longest to mean read (5/4 and
81/64 sit on either side of the ragged predicate) x both presets x 8 option sets.  tools/make_event_plan_table.py
recorded it from the library BEFORE the plan moved into one unit (event_plan.hip); this test asks the built library the
same questions and demands equality in every column.  The table is never rebuilt here: a planning rule that is meant to
change is recorded again with the tool, on purpose.  (Without a GPU the plan assumes 256 CUs, the MI355X's count, so
the table holds on both machines.)"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_event_plan_table", os.path.join(ROOT, "tools", "make_event_plan_table.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def table():
    with np.load(os.path.join(ROOT, "tests", "golden", "event_plan_table.npz")) as z:
        return {k: z[k] for k in ("inputs", "options", "params", "outputs")}


def test_the_fixture_is_the_whole_grid_and_takes_every_branch(tool, table):
    """a truncated or degenerate fixture cannot pass: the grid is the tool's, and every branch of the plan is in it"""
    inputs, options, params = tool.grid()
    assert len(inputs) == 15600
    assert np.array_equal(table["inputs"], inputs) and table["inputs"].dtype == np.uint64
    assert np.array_equal(table["options"], options) and np.array_equal(table["params"], params)
    out = table["outputs"]
    assert out.shape == (15600, len(tool.COLUMNS)) and out.dtype == np.uint64
    col = {k: out[:, i] for i, k in enumerate(tool.COLUMNS)}
    assert int((col["tail_segment_len"] > 0).sum()) >= 3576
    assert int((col["lanes_per_short_read"] > 0).sum()) >= 1347
    assert int((col["max_segments"] > 0).sum()) >= 7960
    assert len(set(col["long_min"].tolist())) >= 25
    assert set(col["lanes_per_short_read"].tolist()) >= {0, 4, 8, 16, 32}
    # the two routes size different workspaces, and the presets' kernels take sgk_event_opt's
    assert np.array_equal(col["workspace_bytes_param_preset_kernels"], col["workspace_bytes_opt"])
    assert (col["workspace_bytes_param_generic"] != col["workspace_bytes_opt"]).any()
    assert (col["workspace_bytes_opt"] > 0).all() and (col["workspace_bytes_param_generic"] > 0).all()


def test_every_row_is_the_recorded_one(tool, table):
    from sigtk_amd import api
    got = tool.answers(api.load_library(), table["inputs"], table["options"], table["params"])
    want = table["outputs"]
    bad = np.argwhere(got != want)
    msg = ""
    if len(bad):
        i, j = (int(x) for x in bad[0])
        msg = "%d cells differ; first: row %d %s (options %s), column %s: got %d, recorded %d" % (
            len(bad), i, table["inputs"][i].tolist(), table["options"][int(table["inputs"][i][4])].tolist(),
            tool.COLUMNS[j], int(got[i, j]), int(want[i, j]))
    assert not len(bad), msg
