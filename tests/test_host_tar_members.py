"""znippy_archive_extract_tar_members (the compiled host layer): the Cargo.toml of every archived .crate in one batch — the heads of the
files gathered on the device, znippy_targz_find_batch on them there, the whole file only where the head did not hold the answer —
against tarfile's reading of the same crates.  The archive is written by host.compress_dir, once with the crates stored (the
extension rule) and once with no_skip, so that they are compressed rows."""
import gzip
import io
import tarfile

import pytest

import gen

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_NOENT = 0, -1, -4, -5, -9


def manifest(i):
    n = 200 + (i * 997) % 3000
    deps = b"".join(b"dep%d = { version = \"%d.%d\", features = [\"f%d\"] }\n" % (k, k % 7, i % 11, k) for k in range(120))
    return (b"[package]\nname = \"crate%d\"\nversion = \"1.0.%d\"\n\n[dependencies]\n" % (i, i) + deps)[:n]


def make_crate(i, cargo="second", big=False):
    """GNU format, as cargo package writes it; the manifest second, last (behind more than 64 KiB of compressed source) or absent"""
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.GNU_FORMAT) as tf:
        def add(name, data):
            ti = tarfile.TarInfo(f"crate{i}-1.0.{i}/{name}")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
        add(".cargo_vcs_info.json", b'{"git":{"sha1":"%040x"}}' % i)
        if cargo == "second":
            add("Cargo.toml", manifest(i))
        for k in range(1 + i % 3):
            add(f"src/m{k}.rs", gen.pseudo_text(2000 + 3111 * k + 50 * i, seed=i + k))
        if big:
            add("assets/noise.bin", gen.incompressible(i, 150_000))
        if cargo == "last":
            add("Cargo.toml", manifest(i))
    return gzip.compress(b.getvalue(), 6, mtime=0)


@pytest.fixture(scope="module")
def crates():
    files = {f"index/cr/at/crate{i}-1.0.{i}.crate": make_crate(i) for i in range(30)}
    files["index/late.crate"] = make_crate(100, cargo="last", big=True)     # the answer lies behind the head: pass 2
    files["index/none.crate"] = make_crate(101, cargo=None)
    files["index/text.crate"] = gen.text(3000)
    files["sdist/pkg-1.0.tar.gz"] = make_crate(102)
    assert len(files["index/late.crate"]) > 128 << 10
    return files


@pytest.fixture(scope="module")
def archives(crates, tmp_path_factory):
    """no_skip -> (open archive, its path, its index rows), written on first use"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    d = tmp_path_factory.mktemp("tar_members")
    for k, v in crates.items():
        (d / "in" / k).parent.mkdir(parents=True, exist_ok=True)
        (d / "in" / k).write_bytes(v)
    made = {}

    def get(no_skip):
        if no_skip not in made:
            p = d / f"a{int(no_skip)}.znippy"
            host.compress_dir(d / "in", p, no_skip)
            rows = host.read_index(p)[0]
            assert any(r["compressed"] for r in rows if r["relative_path"].endswith(".crate")) == no_skip
            made[no_skip] = (host.ZnippyArchive.open(p), p, rows)
        return made[no_skip]
    yield get
    for a, _, _ in made.values():
        a.close()


@pytest.fixture(scope="module", params=[False, True], ids=["stored", "no_skip"])
def archive(request, archives):
    return archives(request.param)


def expected(crates, path, suffix="/Cargo.toml"):
    if path not in crates:
        return E_INVAL, None
    try:
        with tarfile.open(fileobj=io.BytesIO(crates[path]), mode="r:gz") as tf:
            for ti in tf:
                if ti.isreg() and ti.name.endswith(suffix):
                    return OK, tf.extractfile(ti).read()
    except (tarfile.ReadError, gzip.BadGzipFile):
        return E_CORRUPT, None
    return E_NOENT, None


def check_all(a, crates):
    paths = sorted(crates) + ["index/unknown.crate"]
    got, st = a.extract_tar_members(paths, "/Cargo.toml")
    for p, g, s in zip(paths, got, st):
        want_st, want = expected(crates, p)
        assert s == want_st, (p, s, want_st)
        assert g == want, p
    assert st.count(OK) == 32 and st[paths.index("index/none.crate")] == E_NOENT and st[paths.index("index/text.crate")] == E_CORRUPT and st[-1] == E_INVAL
    return got, st


def test_every_manifest_in_one_batch(archive, crates):
    a, _, _ = archive
    check_all(a, crates)
    paths = sorted(crates)
    # prefix and suffix together; a filter that matches the first member of every crate; one that matches nothing; no file at all
    got, st = a.extract_tar_members(paths[:5], ".toml", prefix="crate")
    assert got == [expected(crates, p)[1] for p in paths[:5]]
    got, st = a.extract_tar_members(["index/cr/at/crate3-1.0.3.crate", "index/late.crate"], ".cargo_vcs_info.json")
    assert st == [OK, OK] and got[0].startswith(b'{"git"') and got[1].startswith(b'{"git"')
    got, st = a.extract_tar_members(paths[:3], ".nothing")
    assert st == [E_NOENT] * 3 and got == [None] * 3
    assert a.extract_tar_members([], "/Cargo.toml") == ([], [])
    # a member that is not complete within scan_cap
    got, st = a.extract_tar_members(["index/late.crate", "index/cr/at/crate3-1.0.3.crate"], "/Cargo.toml", scan_cap=64 << 10)
    assert st == [E_DST_SMALL, OK] and got[1] == expected(crates, "index/cr/at/crate3-1.0.3.crate")[1]


def test_a_short_head_sends_most_files_through_pass_two(archive, crates, monkeypatch):
    a, _, _ = archive
    first = check_all(a, crates)
    monkeypatch.setenv("ZNIPPY_HOST_TARGZ_HEAD", "512")   # read at the call
    assert any(len(v) > 512 for v in crates.values())
    assert check_all(a, crates) == first
    monkeypatch.setenv("ZNIPPY_HOST_TARGZ_HEAD", "1")
    assert check_all(a, crates) == first


def test_cap_one_byte_short(archive, crates):
    a, _, _ = archive
    paths = [p for p in sorted(crates) if expected(crates, p)[0] == OK][:6]
    sizes = [len(expected(crates, p)[1]) for p in paths]
    got, st = a.extract_tar_members(paths, "/Cargo.toml", cap=sum(sizes))
    assert st == [OK] * 6
    got, st = a.extract_tar_members(paths, "/Cargo.toml", cap=sum(sizes) - 1)
    assert st == [OK] * 5 + [E_DST_SMALL] and got[5] is None
    assert got[:5] == [expected(crates, p)[1] for p in paths[:5]]
    # a file in the middle that does not fit leaves the ones in front of it clean
    got, st = a.extract_tar_members(paths, "/Cargo.toml", cap=sum(sizes[:3]) - 1)
    assert st[:2] == [OK, OK] and st[2] == E_DST_SMALL and got[:2] == [expected(crates, p)[1] for p in paths[:2]]
