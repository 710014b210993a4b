"""hsflow.py against the committed call table tests/golden/py_calls.json
(tests/golden/make_py_calls.py wrote it from the binding in front of its
refactor): for every public callable, per case, the C calls it makes -- which
buffer in which slot, every size, code, struct and default workspace size, the
order of the context's get / set / restore calls -- and what it returns; and
for every argument the Python code itself rejects, the HsflowError's status and
text; for flow_bidir_device and flow_interp_bgr_device every pair of those
faults raises the error of the one whose check the table puts first.

A recorder stands in for the library, so nothing is solved or launched.  The
host half needs no GPU; the device half allocates tensors and is marked gpu."""
import json

import pytest

from golden import make_py_calls as gen

with open(gen.TABLE) as _f:
    TABLE = json.load(_f)


@pytest.fixture(scope="module")
def host(hs):
    return gen.host_cases(hs)


@pytest.fixture(scope="module")
def device(hs):
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cases, faults = gen.device_cases(hs, torch)
    return torch.cuda.stream, side, cases, faults


def test_table_covers_every_entry_point(hs, host):
    """A public callable added to hsflow needs a record (or a place in
    gen.NOT_CALLS, the constants and types)."""
    assert sorted(set(TABLE["host"]) | set(TABLE["device"])) == gen.entry_points(hs)
    assert sorted(TABLE["device"]) == sorted(gen.DEVICE_KEYS)
    assert sorted(TABLE["device_errors"]) == sorted(set(gen.DEVICE_KEYS) - {"alloc_workspace"})
    assert sorted(TABLE["device_check_order"]) == sorted(gen.PAIRED)
    assert {k: sorted(v) for k, v in TABLE["host"].items()} == \
        {k: sorted(v) for k, v in host.items()}


def test_the_recorder_leaves_the_library_in_place(hs, host):
    real = hs.lib()
    gen.record(hs, "Context.flow", **host["Context.flow"]["uint8"])
    gen.record(hs, "Context.flow", **host["Context.flow"]["sizes differ"])
    assert hs.lib() is real and hs._lib is real


@pytest.mark.parametrize("key", sorted(TABLE["host"]))
def test_host_calls(hs, host, key):
    for name, case in host[key].items():
        assert gen.record(hs, key, **case) == TABLE["host"][key][name], (key, name)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(TABLE["device"]))
def test_device_calls(hs, device, key):
    on, side, cases, _ = device
    assert sorted(cases[key]) == sorted(TABLE["device"][key])
    with on(side):
        for name, case in cases[key].items():
            assert gen.record(hs, key, **case) == TABLE["device"][key][name], (key, name)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(TABLE["device_errors"]))
def test_device_errors(hs, device, key):
    """Every single fault: nothing called, status and text as the table has
    them ([status, text, the faults that raise it])."""
    on, side, cases, faults = device
    with on(side):
        got = gen.record_faults(hs, cases, {key: faults[key]})
    assert gen.pack_errors(got[key]) == TABLE["device_errors"][key]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(TABLE["device_check_order"]))
def test_device_error_pairs(hs, device, key):
    """Every pair of faults raises the error of the fault whose check stands
    first in the table's order of the call's checks."""
    on, side, cases, faults = device
    with on(side):
        single = gen.record_faults(hs, cases, {key: faults[key]})
        both = gen.record_faults(hs, cases, {key: faults[key]}, pairwise=True)
    assert len(both[key]) == sum(1 for _ in gen.pairs(faults[key])) > 100
    assert gen.check_order(single[key], both[key]) == TABLE["device_check_order"][key]
