"""The Python binding's own checks (capi.py): the typed pointer arguments, the one call path and the frame-count normaliser.  Host
tests: every call here is refused by the binding before the entry runs, or by the entry before it looks at a pointer."""
import ctypes as C
import os

import pytest
import torch

from early_exit_transformer_amd import capi, ctc
from early_exit_transformer_amd.build import LIB_PATH


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def test_device_pointer_slots_take_addresses_and_refuse_the_wrong_tensor(lib):
    """eec_ctc_log_add(a, b, out, n = 0, stream) returns 0 before it looks at a pointer."""
    assert lib.eec_ctc_log_add(None, None, None, 0, None) == 0
    assert lib.eec_ctc_log_add(4096, C.c_void_p(4096), (C.c_float * 2)(), 0, None) == 0
    x = torch.zeros(4, 6)
    for k, (bad, why) in enumerate([(x.to(torch.int32), r"expected a float tensor, got torch\.int32"),
                                    (x.t(), r"expected a contiguous tensor, got strides \(1, 6\)"),
                                    (x.half(), r"expected a float tensor, got torch\.float16"),
                                    (x, r"expected a device tensor, got one on cpu")]):
        args = [None, None, None]
        args[k % 3] = bad
        with pytest.raises(C.ArgumentError, match=rf"argument {k % 3 + 1}: TypeError: {why}"):
            lib.eec_ctc_log_add(*args, 0, None)


@pytest.mark.gpu
def test_device_pointer_slots_take_a_device_tensor(lib):
    x = torch.zeros(4, 6, device="cuda")
    assert lib.eec_ctc_log_add(x, x[1:], x[2], 0, None) == 0
    with pytest.raises(C.ArgumentError, match="argument 2: TypeError: expected a contiguous tensor"):
        lib.eec_ctc_log_add(x, x[:, 1:], x, 0, None)
    with pytest.raises(C.ArgumentError, match=r"argument 2: TypeError: expected a host \(CPU\) tensor, got one on cuda:0"):
        lib.eec_noise_bank_bytes(1, x, None)


def test_host_pointer_slots_take_cpu_tensors(lib):
    """The packers read host memory: eec_noise_bank_bytes sizes an image from one row of four samples; eec_upload_i64 has one slot
    of each kind and refuses n = 0 before it looks at either."""
    samples, n = torch.ones(4), torch.tensor([4], dtype=torch.int32)
    assert lib.eec_noise_bank_bytes(1, samples, n) == lib.eec_noise_bank_bytes(1, samples.numpy().ctypes.data, n.numpy().ctypes.data) > 0
    with pytest.raises(C.ArgumentError, match=r"argument 2: TypeError: expected a float tensor, got torch\.int32"):
        lib.eec_noise_bank_bytes(1, n, n)
    with pytest.raises(C.ArgumentError, match=r"argument 3: TypeError: expected a int32_t tensor, got torch\.int64"):
        lib.eec_noise_bank_bytes(1, samples, n.long())
    values = torch.arange(3)
    assert lib.eec_upload_i64(values, 0, None, None) == 10001  # the host slot took the CPU tensor; the entry refused n
    with pytest.raises(C.ArgumentError, match="argument 3: TypeError: expected a device tensor, got one on cpu"):
        lib.eec_upload_i64(values, 0, values, None)
    image = torch.zeros(8, dtype=torch.uint8)  # a void* slot takes any element type, still contiguous
    assert lib.eec_noise_bank(1, samples, n, image, 8) == 10003  # EEC_ERR_WORKSPACE: the image is too short
    with pytest.raises(C.ArgumentError, match="argument 4: TypeError: expected a contiguous tensor"):
        lib.eec_noise_bank(1, samples, n, image[::2], 8)


def test_frame_counts():
    dev = torch.device("cpu")
    assert ctc._frame_counts("f", "em_len", None, 3, dev) is None
    for dtype in (torch.int32, torch.int64):
        out = ctc._frame_counts("f", "em_len", torch.tensor([[5, 0, 7]], dtype=dtype), 3, dev)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.tolist() == [5, 0, 7]
    big = torch.tensor([2 ** 31 + 5, -2 ** 40, 12])
    for any_dtype in (False, True):  # the callers that used to narrow without clamping wrapped these to 5 and 0
        assert ctc._frame_counts("f", "em_len", big, 3, dev, any_dtype=any_dtype).tolist() == [2 ** 31 - 1, -2 ** 31, 12]
    assert ctc._frame_counts("f", "em_len", torch.tensor([3.0, 1e12, -1e12]), 3, dev, any_dtype=True).tolist() == [3, 2 ** 31 - 1, -2 ** 31]
    assert ctc._frame_counts("f", "em_len", [1, 2, 3], 3, dev).tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="em_len must have 3 entries, got 2"):
        ctc._frame_counts("f", "em_len", torch.tensor([1, 2]), 3, dev)
    with pytest.raises(ValueError, match="em_len must have 3 entries, got 4"):
        ctc._frame_counts("f", "em_len", torch.zeros(4, dtype=torch.int16), 3, dev, any_dtype=True)


def test_a_failing_call_is_reported_under_the_entry_s_own_name(lib):
    with pytest.raises(RuntimeError, match=r"^eec_ctc_log_add failed \(code 10001\): eec_ctc_log_add: n must not be negative"):
        capi.launch("eec_ctc_log_add", "cpu", None, None, None, -1)
    with pytest.raises(RuntimeError, match=r"^eec_greedy_ctc_len failed \(code 10001\)"):
        capi.launch("eec_greedy_ctc_len", "cpu", None, None, 1, 8, 4, 0, None, None)
    with pytest.raises(RuntimeError, match=r"^eec_encoder_create failed \(code 10001\)"):
        capi.call("eec_encoder_create", None, None)
    # the stream goes where the prototype has it, not at the end
    assert lib.eec_ctc_lexbeam_lm_decode.argtypes.index(capi.STREAM) == 23 and len(lib.eec_ctc_lexbeam_lm_decode.argtypes) == 26
    with pytest.raises(RuntimeError, match=r"^eec_ctc_lexbeam_lm_decode failed"):
        capi.launch("eec_ctc_lexbeam_lm_decode", "cpu", None, 1, 8, 4, None, None, 0, -1, 4, 1, 0.0, 0.0, 50.0, 8, *[None] * 8, 0, None, 1.0)
