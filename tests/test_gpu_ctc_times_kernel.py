"""cn_op_ctc_token_times on the device against the serial host entry, and so against the numpy model (tests/ctc_times_model.py): spans,
status, conf and score bit for bit over the whole case list, with the back-pointers in LDS and in device scratch, in both libraries;
sentinels behind every row's labels and behind the batch survive."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_times_cases as cases
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cases.cases()]


def p(t):
    return C.c_void_p(t.data_ptr())


def run_op(c, lib, limit):
    B, Tp, V = c.logp.shape
    dev = [torch.from_numpy(a).cuda() for a in (c.logp, c.frames, c.labels, c.label_len)]
    out = [torch.from_numpy(a).cuda() for a in cases.out_buffers(c)]
    rc = lib.cn_op_ctc_token_times(p(dev[0]), p(dev[1]), p(dev[2]), c.labels.shape[1], p(dev[3]), B, Tp, V, c.blank, int(limit), *(p(t) for t in out),
                                   hip.current_stream())
    assert rc == 0, lib.cn_last_error()
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("limit", [-1, 0], ids=["lds", "scratch"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_host_entry_and_the_model(name, limit, flavour):
    c = cases.case(name)
    lib = hip.lib(flavour)
    got = run_op(c, lib, limit)
    for g, h in zip(got, cases.run_host(c, lib)):
        assert np.array_equal(cases.bits(g), cases.bits(h)), name
    cases.same_as_model(c, got)


@pytest.mark.parametrize("name", ["t7_dyadic", "t40_v5000_b33", "t300_v8"])
def test_the_threshold_argument_switches_the_form_at_tp_times_states(name):
    """At T' * (2 ld + 1) the back-pointers are still in LDS, one below they go to scratch: the same bits on either side."""
    c = cases.case(name)
    at = c.logp.shape[1] * (2 * c.labels.shape[1] + 1)
    for limit in (at, at - 1, 1 << 40):
        cases.same_as_model(c, run_op(c, hip.lib(), limit))
