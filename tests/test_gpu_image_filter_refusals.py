"""Which refusal wins: the walk of tests/image_filter_refusals.py over the image filters' entries, on a context and on a handle over two
contexts, against tests/golden/image_filter_refusals.json — the codes and messages of the library as it was before the filters' host
code became one path, recorded on an MI355X.  Entry for entry: the label, the return code and the text of the message."""
import json
import os

import pytest

import image_filter_refusals

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_filter_refusals.json")


def test_every_refusal_is_the_recorded_one(rtx):
    with open(GOLDEN) as f:
        want = [tuple(e) for e in json.load(f)]
    got = image_filter_refusals.walk(rtx)
    assert [e[0] for e in got] == [e[0] for e in want], "the walk's calls differ from the recorded ones"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} entries differ; the first (got, recorded): {wrong[0]}"
    assert all(rc in (-1, -2) for _, rc, _ in got), "a call of the walk was not refused"
