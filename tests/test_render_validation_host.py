"""What the four whole-ray render entry points and their workspace queries answer to a call that fails a check, against the table recorded
before the entry points were folded into one pipeline (tests/golden/render_validation.json, written by
tests/golden/make_golden_render_validation.py).  No GPU: host memory, every call is refused before any HIP call or has N == 0.
A single fault, alone or in a call with N == 0, reproduces return code and message byte for byte; two faults at once give the same return
code and the message of one of the two."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_render_validation", os.path.join(GOLDEN, "make_golden_render_validation.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
ROWS = G.rows()


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(GOLDEN, "render_validation.json")))


def test_the_table_covers_every_entry_point_and_fault(table):
    keys = set(table["calls"])
    assert keys <= {r[0] for r in ROWS}
    singles = [r for r in ROWS if r[4] is None]
    assert all(r[0] in keys for r in singles) and len(singles) > 250
    assert sum(len(v) == 3 for v in table["calls"].values()) > 200                      # pairs
    for entry, names in G.ARGS.items():
        for variant in G.VARIANTS[entry]:
            for fault, (_, applies) in G.FAULTS.items():
                if applies(entry, variant, names):
                    assert "%s[%s] %s" % (entry, variant, fault) in keys
    for fault in G.FAULTS:                                                             # every fault applies somewhere
        assert any(k.endswith("] " + fault) for k in keys), fault


@pytest.mark.parametrize("entry", list(G.ARGS))
def test_refusals_reproduce_the_recorded_code_and_message(table, entry):
    from nerf_amd import _lib
    calls = table["calls"]
    n = 0
    for key, e, variant, changes, singles in ROWS:
        if e != entry or key not in calls:
            continue
        want = calls[key]
        rc, msg = G.call(_lib, e, variant, changes)
        assert rc == want[0], (key, rc, msg, want)
        if singles is None:
            assert msg == want[1], (key, msg, want)
            assert rc != 0 or changes.get("N") == 0, key
        else:
            assert rc != 0 and msg in (calls[singles[0]][1], calls[singles[1]][1]), (key, msg, want)
        n += 1
    assert n > 60, n


def test_workspace_queries_reproduce_the_recorded_sizes(table):
    from nerf_amd import _lib
    assert G.queries(_lib) == table["queries"]
    assert set(table["queries"]) == set(G.QUERIES)
