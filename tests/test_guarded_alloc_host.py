"""tests/guarded_alloc.py on the CPU: the detector detects, without any access outside memory the test owns.  The two
self-tests write through torch.as_strided one element behind and one element in front of a guarded tensor; both land in
the guard band, which belongs to the same backing storage.

Backward threads: on this torch (2.10) the dispatch mode is part of the thread-local state that autograd hands to its
worker threads.  For CPU tensors backward runs on the calling thread, which is what the count below shows; the device
thread is checked by tests/test_gpu_guard_bands.py::test_detector_on_the_gpu."""
import numpy as np
import pytest
import torch

from tests.guarded_alloc import Guarded

DTYPES = [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.int16, torch.bool]


def test_write_one_element_behind_is_caught_and_named():
    n = 37                                                     # 148 bytes: no multiple of anything an allocator rounds to
    with Guarded(devices=("cpu",)) as g:
        t = torch.empty(n, dtype=torch.float32)
        g.check()
        torch.as_strided(t, (n + 1,), (1,))[n] = 1.0
        with pytest.raises(AssertionError) as e:
            g.check()
    msg = str(e.value)
    assert g.count == 1
    assert "BEHIND" in msg and "aten.empty.memory_format" in msg and "float32[37]" in msg
    assert "test_guarded_alloc_host.py" in msg and "test_write_one_element_behind_is_caught_and_named" in msg
    assert "first damaged offset %d" % (4 * n) in msg and "that is 1 byte(s) past" in msg and "4 byte(s) damaged" in msg


def test_write_one_element_in_front_is_caught_and_named():
    n = 5
    with Guarded(devices=("cpu",)) as g:
        keep = torch.zeros(3)                                  # an undamaged neighbour is not named
        t = torch.full((n,), 2, dtype=torch.int16)
        front = torch.as_strided(t, (n + 1,), (1,), t.storage_offset() - 1)
        front[0] = 7
        with pytest.raises(AssertionError) as e:
            g.check()
    msg = str(e.value)
    assert g.count == 2 and keep.tolist() == [0, 0, 0] and t.tolist() == [2] * n
    assert "FRONT" in msg and "aten.full" in msg and "int16[5]" in msg and "aten.zeros" not in msg
    assert "first damaged offset -2" in msg and "nearest 1 byte(s) before" in msg


def test_a_read_only_pass_leaves_the_guards_alone():
    with Guarded(devices=("cpu",)) as g:
        t = torch.zeros(100)
        assert float((t + 1).sum()) == 100.0
        g.check()
    assert g.count == 1


@pytest.mark.parametrize("poison", [0xFF, 0x00, 0xA5])
def test_filled_factories_keep_their_values_and_empty_is_poisoned(poison):
    with Guarded(poison=poison, devices=("cpu",)) as g:
        z = torch.zeros(3, 5)
        zl, nz = torch.zeros_like(z, dtype=torch.int32), z.new_zeros(7)
        o = torch.ones(4, dtype=torch.float64)
        f, fl, nf = torch.full((2, 3), 2.5), torch.full_like(z, -1.0), z.new_full((3,), 9.0)
        e, es = torch.empty(11, dtype=torch.int32), torch.empty_strided((2, 3), (3, 1), dtype=torch.uint8)
        el, ne = torch.empty_like(z), z.new_empty(2, dtype=torch.int64)
        g.check()
    assert g.count == 11
    for t in (z, zl, nz):
        assert not t.any()
    assert o.tolist() == [1.0] * 4 and (f == 2.5).all() and (fl == -1.0).all() and (nf == 9.0).all()
    for t in (e, es, el, ne):
        assert (t.contiguous().view(-1).view(torch.uint8) == poison).all()
    if poison == 0xFF:
        assert torch.isnan(el).all() and (e == -1).all() and (ne == -1).all() and (es == 255).all()


def test_upload_rule_keeps_the_values():
    """An upload is aten._to_copy whose result is on a guarded device and whose source is not.  There is no second device
    here, so the rule's two halves are shown apart: a copy within the guarded device passes through, and the path an
    upload takes (_guard with keep=True) returns the source's values between intact bands."""
    src = torch.from_numpy(np.arange(13, dtype=np.float32))
    with Guarded(devices=("cpu",)) as g:
        same = src.to(torch.float64)
        assert g.count == 0 and same.tolist() == src.tolist()
    up = g._guard(src.to(torch.float64), torch.ops.aten._to_copy.default, keep=True)   # as from inside the dispatch
    g.check()
    assert g.count == 1 and up.dtype == torch.float64 and up.tolist() == src.tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(1,), (37,), (3, 5, 7), (2, 1, 129)], ids=str)
def test_dtype_shape_contiguity_and_alignment_are_kept(dtype, shape):
    with Guarded(devices=("cpu",)) as g:
        t = torch.empty(shape, dtype=dtype)
        z = torch.zeros(shape, dtype=dtype)
    assert g.count == 2
    for x in (t, z):
        assert x.dtype == dtype and tuple(x.shape) == shape and x.is_contiguous() and x.data_ptr() % 16 == 0
        assert x.stride() == torch.empty(shape).stride()
    rec = g.records[0]
    assert rec.nbytes == t.numel() * t.element_size()          # the back band begins at the exact size: no rounding
    assert t.data_ptr() == rec.raw.data_ptr() + g.guard and rec.raw.numel() == 2 * g.guard + rec.nbytes


def test_what_is_not_guarded_passes_through():
    with Guarded(devices=("cpu",)) as g:
        a = torch.empty(0)                                     # zero elements
        b = torch.empty_strided((3, 4), (1, 3))                # not contiguous
        c = torch.empty(2, 3, 4, 5).to(memory_format=torch.channels_last)
        n = g.count
        d = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        e = torch.arange(5) + 1                                # not a factory of the list
    assert n == 1 and g.count == 1                             # only the contiguous empty(2, 3, 4, 5) in c's line
    assert a.numel() == 0 and b.stride() == (1, 3) and d.is_contiguous(memory_format=torch.channels_last)
    assert c.shape == d.shape and e.tolist() == [1, 2, 3, 4, 5]
    with Guarded(devices=("cuda",)) as g:                      # another device's mode leaves CPU tensors alone
        torch.zeros(4)
    assert g.count == 0


def test_tensor_made_inside_backward_is_guarded():
    made = []

    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty_like(x)
            torch.mul(x, 2.0, out=out)
            return out

        @staticmethod
        def backward(ctx, go):
            gi = torch.empty_like(go)
            made.append(gi.clone())
            torch.mul(go, 2.0, out=gi)
            return gi

    x = torch.arange(6, dtype=torch.float32).requires_grad_(True)
    go = torch.ones(6)
    with Guarded(devices=("cpu",)) as g:
        y = Twice.apply(x)
        before = g.count
        y.backward(go)
        g.check()
    assert before == 1 and g.count == 2                        # forward's empty_like, then backward's
    assert g.records[1].op.startswith("aten.empty_like") and "backward" in g.records[1].where
    assert torch.isnan(made[0]).all()                          # it arrived poisoned
    assert x.grad.tolist() == [2.0] * 6 and y.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0]
