"""Helpers of the GPU tests of znippy_tar_list_batch: one call over tars placed in device memory, with guard bytes around everything
the call may write, in the shape of tar_list_model.batch.  Not a test file."""
import ctypes as C

import numpy as np

import tar_list_model as M

GUARD = 0xA5
PAD = 64


def place(tars, odd=True):
    """the tars back to back with gaps of filler in between: (bytes, offsets) — odd: every item starts at an odd address offset"""
    buf, offs = bytearray(b"\xEE" * (3 if odd else 0)), []
    for i, t in enumerate(tars):
        if odd and len(buf) % 2 == 0:
            buf += b"\xEE"
        offs.append(len(buf))
        buf += t
        buf += b"\xEE" * ((5 + 2 * (i % 7)) if odd else (-len(buf) % 512))
    return bytes(buf) + b"\xEE" * 16, offs


def call(ctx, d_tar, offs, lens, prefix=b"", suffix=b"", contents=True, members_cap=None, names_cap=None, out_cap=None, measure=False, tar_cap=None):
    """One call.  Caps of None: what a measuring call reports.  Returns (status, member_first, members, names, out, names_bytes,
    out_bytes, rc) with members as (item, header_off, data_off, size, name, typeflag, name_off, out_off); the guards are checked."""
    import torch
    from znippy_amd import hip
    from znippy_amd._lib import np_ptr
    n = len(offs)
    to, tl = np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    tar_cap = d_tar.numel() if tar_cap is None else tar_cap
    status = np.full(max(n, 1), 77, dtype=np.int32)
    first = np.full(n + 1, 77, dtype=np.uint64)
    nb, ob = C.c_uint64(77), C.c_uint64(77)
    dptr = C.c_void_p(d_tar.data_ptr())
    if measure or None in (members_cap, names_cap) or (contents and out_cap is None):
        rc = ctx.L.znippy_tar_list_batch(ctx.h, dptr, tar_cap, np_ptr(to), np_ptr(tl), n, prefix, len(prefix), suffix, len(suffix), None, 0, None, 0, None, 0,
                                         np_ptr(first), C.byref(nb), C.byref(ob), np_ptr(status))
        if measure:
            return [int(s) for s in status[:n]], [int(f) for f in first], [], b"", b"", nb.value, ob.value, rc
        assert rc == 0
        members_cap = int(first[n]) if members_cap is None else members_cap
        names_cap = nb.value if names_cap is None else names_cap
        out_cap = ob.value if out_cap is None else out_cap
    members = np.frombuffer(bytes([GUARD]) * (hip.TAR_MEMBER.itemsize * (members_cap + 4)), dtype=hip.TAR_MEMBER).copy()
    names = np.full(names_cap + PAD, GUARD, dtype=np.uint8)
    d_out = torch.full((PAD + out_cap + PAD,), GUARD, dtype=torch.uint8, device="cuda") if contents else None
    torch.cuda.synchronize()
    rc = ctx.L.znippy_tar_list_batch(ctx.h, dptr, tar_cap, np_ptr(to), np_ptr(tl), n, prefix, len(prefix), suffix, len(suffix), np_ptr(members), members_cap,
                                     np_ptr(names), names_cap, C.c_void_p(d_out.data_ptr() + PAD) if contents else None, out_cap if contents else 0,
                                     np_ptr(first), C.byref(nb), C.byref(ob), np_ptr(status))
    st, fi = [int(s) for s in status[:n]], [int(f) for f in first]
    if rc:
        return st, fi, [], b"", b"", nb.value, ob.value, rc
    total = fi[n]
    assert total <= members_cap and nb.value <= names_cap and (not contents or ob.value <= out_cap)
    # nothing outside what is reported has been written
    assert (members[total:].view(np.uint8) == GUARD).all(), "entries of members behind the reported ones were written"
    assert (names[nb.value:] == GUARD).all(), "bytes of names behind the reported ones were written"
    out = b""
    if contents:
        whole = d_out.cpu().numpy()
        assert (whole[:PAD] == GUARD).all() and (whole[PAD + ob.value:] == GUARD).all(), "bytes of d_out outside the reported ones were written"
        out = whole[PAD:PAD + ob.value].tobytes()
    nm = names[:nb.value].tobytes()
    ms = []
    for i in range(n):
        for j in range(fi[i], fi[i + 1]):
            m = members[j]
            ms.append((i, int(m["header_off"]), int(m["data_off"]), int(m["size"]), nm[int(m["name_off"]):int(m["name_off"]) + int(m["name_len"])], int(m["typeflag"]),
                       int(m["name_off"]), int(m["out_off"])))
    return st, fi, ms, nm, out, nb.value, ob.value, rc


def run_batch(ctx, tars, prefix=b"", suffix=b"", odd=True, **kw):
    import torch
    buf, offs = place(tars, odd)
    d_tar = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    return call(ctx, d_tar, offs, [len(t) for t in tars], prefix, suffix, **kw)


def expect(tars, prefix=b"", suffix=b"", contents=True, **caps):
    """what run_batch returns for whole tars, by the model (rc 0)"""
    st, first, members, names, out = M.batch(tars, prefix, suffix, **caps)
    return st, first, members, names, (out if contents else b""), len(names), len(out), 0
