"""tests/offset_views.py on CPU tensors and arrays: the values, the contiguity and the pointer residues the GPU alignment tests
(tests/test_gpu_pointer_alignment.py) rely on.  Needs no GPU."""
import numpy as np
import pytest

from tests.offset_views import PAD, offset_array, offset_view, residue

DTYPES = ["float32", "int32", "uint8", "float64"]
SHAPES = [(7,), (5, 9), (4, 3, 5)]


def values(dtype, shape):
    rs = np.random.RandomState(len(shape))
    a = rs.randint(1, 200, shape)
    return a.astype(dtype) if dtype in ("int32", "uint8") else (a + rs.rand(*shape)).astype(dtype)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("dtype", DTYPES)
def test_offset_array(dtype, k, shape):
    a = values(dtype, shape)
    keep = a.copy()
    v = offset_array(a, k)
    assert v.dtype == a.dtype and v.shape == a.shape and v.flags["C_CONTIGUOUS"]
    assert np.array_equal(v, keep) and np.array_equal(a, keep)
    base = v.base
    while base.base is not None:
        base = base.base
    assert base.size == a.size + k + PAD
    assert v.ctypes.data - base.ctypes.data == k * a.itemsize
    assert residue(v) == (residue(base) + k * a.itemsize) % 16
    assert residue(v, 4) == (residue(base, 4) + k * a.itemsize) % 4
    # NumPy's allocations start on a 16-byte boundary: the residues are the ones the GPU tests name
    assert residue(base) == 0 and residue(v) == (k * a.itemsize) % 16
    assert not base[:k].any() and not base[k + a.size:].any()
    # ascontiguousarray, what the wrappers call, hands the same memory on
    assert np.ascontiguousarray(v, dtype=a.dtype).ctypes.data == v.ctypes.data


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("dtype", DTYPES)
def test_offset_view(dtype, k, shape):
    torch = pytest.importorskip("torch")
    a = values(dtype, shape)
    t = torch.as_tensor(a.copy())
    v = offset_view(t, k)
    assert v.dtype == t.dtype and tuple(v.shape) == shape and v.is_contiguous()
    assert np.array_equal(v.numpy(), a) and np.array_equal(t.numpy(), a)
    assert v.storage_offset() == k
    store = v.untyped_storage()
    assert store.nbytes() == (a.size + k + PAD) * a.itemsize
    assert v.data_ptr() - store.data_ptr() == k * a.itemsize
    assert residue(v) == (store.data_ptr() + k * a.itemsize) % 16
    assert store.data_ptr() % 16 == 0 and residue(v) == (k * a.itemsize) % 16
    assert residue(v, 4) == (k * a.itemsize) % 4
    # .to(dtype).contiguous(), what the wrappers call, hands the same memory on
    assert v.to(t.dtype).contiguous().data_ptr() == v.data_ptr()
    flat = torch.zeros(0, dtype=t.dtype).set_(store)
    assert not flat[:k].any() and not flat[k + a.size:].any()


def test_the_offsets_the_gpu_tests_use_give_the_residues_they_name():
    f32 = np.zeros(8, np.float32)
    assert [residue(offset_array(f32, k)) for k in (1, 2, 3)] == [4, 8, 12]
    u8 = np.zeros(8, np.uint8)
    assert [residue(offset_array(u8, k), 4) for k in (1, 2, 3, 5)] == [1, 2, 3, 1]
    assert residue(offset_array(np.zeros(8, np.float64), 1)) == 8
    assert residue(offset_array(np.zeros(8, np.int64), 1)) == 8
