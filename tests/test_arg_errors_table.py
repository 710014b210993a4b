"""Every argument check of the warped family against the committed table
tests/golden/arg_errors.json (tests/golden/make_arg_errors.py wrote it from
the library in front of the host-layer refactor): the status of every call
with one invalid argument and its hsflow_last_error text with the digits
normalised; for the four *_sm_device solves every pair of those faults too,
whose text is one of the two faults' own.

CPU only.  Every case fails a check, so no call reaches a launch -- but a
check dropped by mistake would, on invented addresses; where a GPU is visible
the tests therefore skip themselves."""
import json
import re

import pytest
import torch

from golden import make_arg_errors as gen

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="invented device addresses: only where no GPU is visible")

with open(gen.TABLE) as _f:
    TABLE = json.load(_f)


def _values_masked(text):
    """A normalised text with every printed value (-N, N.N, Ne+N, nan, inf) as N."""
    return re.sub(r"-?\b(N(\.N)?(e[+-]N)?|nan|inf)\b", "N", text)


@pytest.fixture(scope="module")
def family(hs):
    return gen.calls(hs)


def test_table_covers_the_generators_cases(hs, family):
    assert TABLE["status"] == hs.HSFLOW_ERR_ARG  # only failing cases are in the table
    assert sorted(TABLE["single"]) == sorted(family)
    for name, (_, faults) in family.items():
        assert sorted(gen.single_texts(TABLE, name)) == sorted(faults), name
    assert sorted(TABLE["pairs"]) == sorted(gen.PAIRED)
    for name in gen.PAIRED:
        assert TABLE["pairs"][name] == sum(1 for _ in gen.pairs(family[name][1])), name
    assert sorted(TABLE["host_null_context"]) == sorted(gen.host_calls())


@pytest.mark.parametrize("name", sorted(TABLE["single"]))
def test_single_faults(hs, family, name):
    params, faults = family[name]
    for fault, text in gen.single_texts(TABLE, name).items():
        assert gen.run(hs, name, params, faults[fault]) == (TABLE["status"], text), (name, fault)


@pytest.mark.parametrize("name", sorted(TABLE["pairs"]))
def test_pairs_of_faults(hs, family, name):
    params, faults = family[name]
    single = gen.single_texts(TABLE, name)
    for a, b, both in gen.pairs(faults):
        status, text = gen.run(hs, name, params, both)
        assert status == TABLE["status"], (name, a, b)
        ta, tb = single[a], single[b]
        if text in (ta, tb):
            continue
        # one check that echoes both arguments (the thresholds' "rel %g, abs
        # %g"): with both invalid its text holds both bad values, so it is
        # neither fault's own text.  Then the two faults' texts are the same
        # message but for the values, and so must this one be.
        assert _values_masked(ta) == _values_masked(tb) == _values_masked(text), \
            (name, a, b, text)


def test_host_forms_with_a_null_context(hs):
    L = hs.lib()
    for name, args in gen.host_calls().items():
        assert getattr(L, name)(*args) == TABLE["status"], name
        text = TABLE["host_null_context"][name]
        if text is not None:
            assert gen.normalise(L.hsflow_last_error(None).decode()) == text, name
