"""The guard-band helper (tests/redzone.py) proven on CPU tensors: a harness that cannot fail is worse than none.
Each negative case plants exactly the defect the corresponding check exists for and expects the AssertionError and its wording."""
import pytest
import torch

import redzone
from redzone import assert_guards, assert_written, guard_report, guarded, guarded_like, guarded_workspace

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8]


def _raw(t):
    z = t._redzone
    return z.alloc, z.off, z.nbytes


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_alignment_guard_size_and_fill(dtype):
    t = guarded((5, 7, 100), dtype, "cpu")
    alloc, off, nbytes = _raw(t)
    item = t.element_size()
    pitch = 100 * item
    want = max(64 << 10, redzone.GUARD_ROWS * pitch)
    want = (want + 4095) // 4096 * 4096
    assert t.is_contiguous() and t.shape == (5, 7, 100) and t.dtype == dtype
    assert t.data_ptr() % 4096 == 0 and t.data_ptr() == alloc.data_ptr() + off
    assert nbytes == 5 * 7 * 100 * item
    assert off >= want and alloc.numel() - off - nbytes >= want             # either guard: at least GUARD_ROWS rows / 64 KiB
    assert bool((alloc[:off] == 0xFF).all()) and bool((alloc[off + nbytes:] == 0xFF).all())
    assert bool((alloc[off:off + nbytes] == 0xFF).all())                      # body="nan"
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())                                     # the pattern is NaN in every float type used here ...
    elif dtype != torch.uint8:
        assert bool((t == -1).all())                                          # ... and -1 in the integer types
    assert guard_report(t) is None
    assert redzone.unwritten(t)[0] == t.numel()


def test_wide_rows_get_twice_the_tallest_tile_of_guard():
    assert redzone.GUARD_ROWS == 384                                          # 2 x the 192-pixel tile of conv3x3h's 6-row form
    t = guarded((3, 1024), torch.float32, "cpu")                              # pitch 4 KiB -> 1.5 MiB on either side
    alloc, off, nbytes = _raw(t)
    assert off >= 384 * 4096 and alloc.numel() - off - nbytes >= 384 * 4096
    t2 = guarded((3, 100), torch.bfloat16, "cpu", pitch_bytes=1024)           # explicit pitch
    assert t2._redzone.pitch == 1024 and t2._redzone.off >= 384 * 1024


def test_exact_write_is_silent():
    t = guarded((9, 100), torch.bfloat16, "cpu")
    t.copy_(torch.randn(9, 100))
    assert_guards(t, "exact")
    assert_written(t, what="exact")
    ws = guarded_workspace(1000, "cpu")
    assert ws.numel() == 1000 and ws.dtype == torch.uint8
    ws.zero_()
    assert_guards(ws, "workspace")


def test_keep_body_and_copy():
    src = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    t = guarded_like(src, "cpu")
    assert torch.equal(t, src)
    assert_guards(t, "copy")
    assert_written(t)


@pytest.mark.parametrize("where", ["last", "first", "middle"])
def test_one_byte_in_the_front_guard(where):
    t = guarded((9, 100), torch.bfloat16, "cpu")                              # pitch 200 bytes
    alloc, off, nbytes = _raw(t)
    t.zero_()
    at = {"last": off - 1, "first": 0, "middle": off - 200 - 8}[where]
    alloc[at] = 0
    rep = guard_report(t)
    assert len(rep) == 1 and rep[0]["side"] == "front" and rep[0]["count"] == 1
    assert rep[0]["first"] == rep[0]["last"] == at - off                      # negative: bytes in front of the body
    assert rep[0]["first_rows_bytes"] == divmod(at - off, 200)
    with pytest.raises(AssertionError) as e:
        assert_guards(t, "y")
    msg = str(e.value)
    assert msg.startswith("y: front guard touched at ")
    if where == "last":
        assert "at -1 rows +199 bytes (byte -1)" in msg
    if where == "middle":
        assert "at -2 rows +192 bytes (byte -208)" in msg


@pytest.mark.parametrize("where", ["first", "last", "row"])
def test_one_byte_in_the_rear_guard(where):
    t = guarded((9, 100), torch.bfloat16, "cpu")
    alloc, off, nbytes = _raw(t)
    t.zero_()
    end = off + nbytes
    at = {"first": end, "last": alloc.numel() - 1, "row": end + 192}[where]
    alloc[at] = 0x7F
    rep = guard_report(t)
    assert len(rep) == 1 and rep[0]["side"] == "rear" and rep[0]["count"] == 1 and rep[0]["first"] == at - end
    with pytest.raises(AssertionError) as e:
        assert_guards(t, "y")
    msg = str(e.value)
    assert msg.startswith("y: rear guard touched at ")
    if where == "first":
        assert "at +0 rows +0 bytes (byte +0)" in msg
    if where == "row":
        assert "rear guard touched at +0 rows +192 bytes" in msg


def test_a_row_behind_the_last_reports_first_and_last_byte_and_both_sides():
    t = guarded((9, 100), torch.bfloat16, "cpu")
    alloc, off, nbytes = _raw(t)
    end = off + nbytes
    alloc[end + 200:end + 400] = 0                                            # row M + 1, whole
    alloc[off - 8:off] = 0                                                    # and four elements in front of row 0
    rep = {r["side"]: r for r in guard_report(t)}
    assert rep["rear"]["count"] == 200 and rep["rear"]["first_rows_bytes"] == (1, 0) and rep["rear"]["last_rows_bytes"] == (1, 199)
    assert rep["front"]["count"] == 8 and rep["front"]["first"] == -8 and rep["front"]["last"] == -1
    with pytest.raises(AssertionError) as e:
        assert_guards(t, "y")
    assert "front guard touched at -1 rows +192 bytes (byte -8) .. -1 rows +199 bytes (byte -1), 8 bytes changed" in str(e.value)
    assert "rear guard touched at +1 rows +0 bytes (byte +200) .. +1 rows +199 bytes (byte +399), 200 bytes changed" in str(e.value)


def test_writing_the_fill_value_back_is_invisible_by_design():
    """The one blind spot: a stray store of 0xFF bytes.  Outputs of the kernels under test are never all-ones patterns."""
    t = guarded((4, 8), torch.float32, "cpu")
    alloc, off, nbytes = _raw(t)
    alloc[off + nbytes] = 0xFF
    assert guard_report(t) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_element_is_detected(dtype):
    t = guarded((6, 10), dtype, "cpu")
    full = torch.ones(6, 10).to(dtype)
    t.copy_(full)
    assert_written(t)
    t2 = guarded((6, 10), dtype, "cpu")
    t2[:, :9] = full[:, :9]
    t2[:4, 9] = full[:4, 9]                                                   # (4, 9) and (5, 9) never written
    assert redzone.unwritten(t2) == (2, (4, 9))
    with pytest.raises(AssertionError) as e:
        assert_written(t2, what="y")
    assert "y: 2 element(s)" in str(e.value) and "(4, 9)" in str(e.value)
    assert_written(t2, valid=(slice(None), slice(0, 9)))                      # the region that WAS written passes
    assert_written(t2, valid=(slice(0, 4),))
    with pytest.raises(AssertionError):
        assert_written(t2, valid=(slice(4, 6), slice(9, 10)))
    mask = torch.ones(6, 10, dtype=torch.bool)
    mask[4:, 9] = False
    assert_written(t2, valid=mask)                                            # boolean masks select the region too


def test_partly_written_element_counts_as_written_only_if_a_byte_changed():
    t = guarded((4,), torch.float32, "cpu")
    alloc, off, _ = _raw(t)
    alloc[off + 4] = 0                                                        # one byte of element 1
    assert redzone.unwritten(t) == (3, (0,))


def test_views_do_not_pretend_to_be_guarded():
    t = guarded((4, 8), torch.float32, "cpu")
    with pytest.raises(TypeError):
        assert_guards(t[1:], "view")
