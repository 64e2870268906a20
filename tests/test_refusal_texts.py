"""The status and the whole last-error text of every refusal of an image argument (tests/refusal_texts.py) against the record
taken before the api_*.cpp units came to share their argument checks (tests/golden/refusal_texts.json): which of two faults is
reported, under which name, in which words. The tests of each pass assert the status and a part of the text only."""
import json

import pytest

from tests import refusal_texts


def compare(part, collected):
    with open(refusal_texts.GOLDEN) as f:
        recorded = json.load(f)[part]
    assert sorted(collected) == sorted(recorded), "the cases collected and the cases of the record are not the same cases"
    assert all(status < 0 for status, _ in recorded.values())
    different = {key: (collected[key], recorded[key]) for key in recorded if collected[key] != recorded[key]}
    assert not different, different


def test_host_refusals_read_as_recorded():
    compare("host", refusal_texts.collect_host())


@pytest.mark.gpu
def test_pipeline_refusals_read_as_recorded():
    compare("gpu", refusal_texts.collect_gpu())
