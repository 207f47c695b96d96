"""The workspace sizes of the five analyses over resident rows are host arithmetic: every layout's total, recorded in
tests/golden/rows_workspace_bytes.json for the smallest shapes, a row either side of each segment or chunk constant, 2 000 000 x 768 and
the refused arguments (-1), is what the library returns.  A piece that moved or changed its rounding shows here, without a GPU."""
import json
import os

import pytest

from cbas_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_workspace_bytes.json")
with open(GOLDEN) as f:
    TABLE = json.load(f)
NAMES = ("cbas_rows_search_workspace_bytes", "cbas_rows_knn_workspace_bytes", "cbas_rows_kmeans_workspace_bytes",
         "cbas_rows_probe_workspace_bytes", "cbas_rows_pca_workspace_bytes")


def test_the_table_covers_the_five():
    assert sorted(TABLE) == sorted(NAMES)
    for name in NAMES:
        sizes = [case["bytes"] for case in TABLE[name]]
        assert sum(s == -1 for s in sizes) >= 5 and sum(s > 0 for s in sizes) >= 8 and all(s == -1 or s % 16 == 0 for s in sizes), name
        assert any(case["args"][0] == 2_000_000 for case in TABLE[name]), name


@pytest.mark.parametrize("name", NAMES)
def test_workspace_bytes_are_as_recorded(name):
    fn = getattr(_lib.load(), name)
    got = [int(fn(*case["args"])) for case in TABLE[name]]
    assert got == [case["bytes"] for case in TABLE[name]], [(case["args"], case["bytes"], g) for case, g in zip(TABLE[name], got) if g != case["bytes"]]
