"""A Python model of the tar listing (znippy_amd/csrc/tar_list_rules.h) and of znippy_tar_list_batch's room rule, for the CPU test
of the host listing and the GPU tests.  Not a test file.

`listing` is a serial walk written from tarfile's rules, with targz_model's field and pax parsers; tests/test_tar_list_cpu.py pins
it to `tarfile` on valid archives, and the C++ listing and the device to it on damaged ones.  The two deviations from tarfile, both
E_UNSUPPORTED: a pax size= record that differs from the size field of the member behind it (one that equals it is accepted), and
more than EXT_RUN_MAX extended headers in a row."""
import targz_model as T
from targz_model import E_CORRUPT, E_DST_SMALL, E_INVAL, E_UNSUPPORTED, OK  # noqa: F401

REGULAR = (b"0", b"\0", b"7")
EXT_RUN_MAX = 64


def listing(t, prefix=b"", suffix=b""):
    """(status, [(header_off, data_off, size, name, typeflag), ...]): every regular member of the whole tar `t` whose name starts
    with prefix and ends with suffix.  A tar with a status lists nothing."""
    if len(t) >= 1 << 32:
        return E_UNSUPPORTED, []
    h, zeros, run, name, size_over, out = 0, 0, 0, None, None, []
    while True:
        pending = name is not None or size_over is not None
        if h == len(t):
            return (E_CORRUPT, []) if pending else (OK, out)
        if len(t) - h < 512:
            return E_CORRUPT, []
        b = t[h:h + 512]
        if b == bytes(512):
            if pending:
                return E_CORRUPT, []
            zeros += 1
            if zeros == 2:
                return OK, out
            run = 0
            h += 512
            continue
        zeros = 0
        chk = T._number(b[148:156])
        rest = b[:148] + b"        " + b[156:]
        unsigned = sum(rest)
        if chk is None or chk not in (unsigned, unsigned - 256 * (512 - len(rest.translate(None, T.HIGH)))):
            return E_CORRUPT, []
        size = T._number(b[124:136])
        if size is None:
            return E_CORRUPT, []
        typ = b[156:157]
        fname = b[:100].split(b"\0", 1)[0]
        if typ == b"\0" and fname.endswith(b"/"):
            typ = b"5"
        if typ == b"S":
            return E_UNSUPPORTED, []
        step = 512 + (0 if typ in (b"1", b"2", b"3", b"4", b"5", b"6") else (size + 511) // 512 * 512)
        if typ in (b"L", b"x", b"X"):
            if size > 8192:
                return E_UNSUPPORTED, []
            if h + 512 + size > len(t):
                return E_CORRUPT, []
            p = t[h + 512:h + 512 + size]
            path = psize = None
            if typ == b"L":
                path = p.split(b"\0", 1)[0]
            else:
                st, path, psize = T._pax(p)
                if st:
                    return st, []
        if h + step > len(t):
            return E_CORRUPT, []  # the member, or its padding, is cut short
        if typ in (b"L", b"x", b"X", b"g", b"K"):
            run += 1
            if run > EXT_RUN_MAX:
                return E_UNSUPPORTED, []  # a run of extended headers longer than a member looks back
        else:
            run = 0
        if typ in (b"L", b"x", b"X"):
            if path is not None and name is None:
                name = path
            if psize is not None and size_over is None:
                size_over = psize
        elif typ not in (b"g", b"K"):
            if size_over is not None and size_over != size:
                return E_UNSUPPORTED, []
            if typ in REGULAR:
                pfx = b[345:500].split(b"\0", 1)[0]
                full = name if name is not None else (pfx + b"/" + fname if pfx else fname)
                if full.startswith(prefix) and full.endswith(suffix):
                    out.append((h, h + 512, size, full, typ[0]))
            name = size_over = None
        h += step


def batch(tars, prefix=b"", suffix=b"", members_cap=None, names_cap=None, out_cap=None):
    """The call over whole tars (bytes each): (status per item, member_first, members — (item, header_off, data_off, size, name,
    typeflag, name_off, out_off) —, names, contents).  A cap of None holds everything."""
    st, first, members, names, out = [], [0], [], b"", b""
    for i, t in enumerate(tars):
        s, ms = listing(t, prefix, suffix)
        nb, ob = sum(len(m[3]) for m in ms), sum(m[2] for m in ms)
        if s == OK and ((members_cap is not None and len(members) + len(ms) > members_cap) or (names_cap is not None and len(names) + nb > names_cap) or
                        (out_cap is not None and len(out) + ob > out_cap)):
            s, ms = E_DST_SMALL, []
        if s == OK:
            for (h, d, size, name, typ) in ms:
                members.append((i, h, d, size, name, typ, len(names), len(out)))
                names += name
                out += t[d:d + size]
        st.append(s)
        first.append(len(members))
    return st, first, members, names, out
