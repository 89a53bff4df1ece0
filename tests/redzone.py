"""Guard bands around the tensors a kernel launch may touch: did it write ONLY what its contract says?

`guarded(shape, dtype, device)` returns a contiguous tensor that is a view into one larger uint8 allocation:

    [ front guard | body (the tensor) | rear guard ]

Every guard byte is 0xFF -- NaN in fp32 / bf16 / fp16, -1 in the integer types, all bits set in a 64-bit bit vector -- so one pattern serves both
directions: an OUTPUT's guards must still be all 0xFF after the launch (`assert_guards`), and an INPUT read out of range puts NaN into a result, which
the parity assert next to the guard check then sees.  With body="nan" the body carries the same pattern, so that an element the kernel claims to
write and does not is still NaN / -1 afterwards (`assert_written`).

Guard size: max(64 KiB, 384 x row pitch), rounded up to 4 KiB, on either side; the body starts 4 KiB-aligned (the alignment a fresh device tensor
has, so that vector accesses behave as they do in production).  384 rows is twice the tallest pixel tile in the library: the LDS-DMA conv kernel's
tiles are 64 or 128 pixels tall, conv3x3h's evaluation form takes 6 x 32 = 192 pixels per block (csrc/conv3x3h.hip, Geo<6>), so a tail-tile
overrun of a whole tile lands inside the test's own allocation, where it is seen and harms nobody.

The helper is device-agnostic (tests/test_redzone.py proves it on CPU tensors)."""
import math

import torch

FILL = 0xFF
PAGE = 4096
GUARD_MIN = 64 << 10
GUARD_ROWS = 384


def _round_up(n, m):
    return (n + m - 1) // m * m


class _Zone:
    __slots__ = ("alloc", "off", "nbytes", "pitch")

    def __init__(self, alloc, off, nbytes, pitch):
        self.alloc, self.off, self.nbytes, self.pitch = alloc, off, nbytes, pitch


def guarded(shape, dtype, device, pitch_bytes=None, body="nan"):
    """A contiguous tensor of `shape` / `dtype` between two 0xFF guards.  pitch_bytes: the row pitch the guard size and the reports are
    expressed in (default: the last dimension).  body: "nan" = pre-filled with 0xFF (outputs), "keep" = left as allocated, for in-place
    operands and inputs the caller fills (see `guarded_like`)."""
    if body not in ("nan", "keep"):
        raise ValueError(f"guarded: body={body!r}")
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = torch.empty(0, dtype=dtype).element_size()
    nbytes = math.prod(shape) * item
    pitch = int(pitch_bytes) if pitch_bytes else max(item, (shape[-1] if shape else 1) * item)
    guard = _round_up(max(GUARD_MIN, GUARD_ROWS * pitch), PAGE)
    alloc = torch.empty(guard + PAGE + nbytes + guard, dtype=torch.uint8, device=device)
    off = guard + (-(alloc.data_ptr() + guard)) % PAGE           # body start: 4 KiB-aligned, at least `guard` bytes into the allocation
    alloc[:off].fill_(FILL)
    alloc[off + nbytes:].fill_(FILL)
    if body == "nan":
        alloc[off:off + nbytes].fill_(FILL)
    t = alloc[off:off + nbytes].view(dtype).view(shape)
    t._redzone = _Zone(alloc, off, nbytes, pitch)
    return t


def guarded_like(src, device, pitch_bytes=None):
    """`src` copied into a guarded tensor on `device` (an input, or an in-place operand)."""
    t = guarded(src.shape, src.dtype, device, pitch_bytes=pitch_bytes, body="keep")
    t.copy_(src)
    return t


def guarded_workspace(nbytes, device, pitch_bytes=1):
    """Exactly `nbytes` usable bytes (uint8, 0xFF-filled) between guards.  pitch_bytes: the widest row the owner of the workspace carves
    into it (the guards then hold GUARD_ROWS such rows); 1 = the 64 KiB minimum, reports in plain bytes."""
    return guarded((int(nbytes),), torch.uint8, device, pitch_bytes=pitch_bytes, body="nan")


def _zone(t):
    z = getattr(t, "_redzone", None)
    if z is None:
        raise TypeError("not a tensor returned by redzone.guarded() (views of one do not carry the guards)")
    return z


def guard_report(t):
    """None when both guards are intact (one flag crosses to the host); else a list of dicts, one per touched side:
    side ("front" | "rear"), count, first / last (byte offsets of the first and last touched byte: relative to the body's first byte for
    the front guard, hence negative; relative to the byte behind the body for the rear guard, hence >= 0) and, for each of the two,
    (rows, bytes) = divmod(offset, row pitch)."""
    z = _zone(t)
    front, rear = z.alloc[:z.off], z.alloc[z.off + z.nbytes:]
    bad = (front != FILL).any() | (rear != FILL).any()
    if not bool(bad.item()):
        return None
    out = []
    for side, g, base in (("front", front, -z.off), ("rear", rear, 0)):
        idx = (g != FILL).nonzero().flatten()
        if idx.numel():
            first, last = int(idx[0].item()) + base, int(idx[-1].item()) + base
            out.append({"side": side, "count": int(idx.numel()), "first": first, "last": last,
                        "first_rows_bytes": divmod(first, z.pitch), "last_rows_bytes": divmod(last, z.pitch), "pitch": z.pitch})
    return out


def format_report(rep):
    parts = []
    for r in rep:
        (fr, fb), (lr, lb) = r["first_rows_bytes"], r["last_rows_bytes"]
        parts.append(f"{r['side']} guard touched at {fr:+d} rows +{fb} bytes (byte {r['first']:+d}) .. {lr:+d} rows +{lb} bytes (byte {r['last']:+d}), "
                     f"{r['count']} bytes changed, row pitch {r['pitch']} bytes")
    return "; ".join(parts)


def assert_guards(t, what="tensor"):
    """The launch wrote nothing outside `t`: both guards are still all 0xFF."""
    rep = guard_report(t)
    assert rep is None, f"{what}: {format_report(rep)}"


def unwritten(t, valid=None):
    """(count, first index) of the elements of `t[valid]` (valid: an index expression -- slice, tuple of slices, boolean mask --; None = all
    of t) whose bytes are all still 0xFF, i.e. that nothing wrote since guarded(..., body="nan")."""
    r = t if valid is None else t[valid]
    if r.numel() == 0:
        return 0, None
    r = r.contiguous()
    b = r.view(torch.uint8).view(-1, r.element_size())
    miss = (b == FILL).all(dim=1)
    n = int(miss.sum().item())
    if n == 0:
        return 0, None
    flat = int(miss.nonzero()[0].item())
    return n, tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape)) if r.dim() else ()


def assert_written(t, valid=None, what="tensor"):
    """Every element of the region the contract says is written was written (no 0xFF-pattern element is left)."""
    n, first = unwritten(t, valid)
    assert n == 0, f"{what}: {n} element(s) of the region to be written still hold the 0xFF fill, first at index {first} of the region"
