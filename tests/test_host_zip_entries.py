"""znippy_archive_extract_zip_entries (the compiled host layer): the pom.xml of every archived jar in one batch — three range-read
passes, one upload, one znippy_inflate_batch, one copy back — against zipfile's reading of the same jars.  The archive is written by
host.compress_dir, once with the jars stored (the extension rule) and once with no_skip, so that the jars are compressed rows."""
import io
import shutil
import zipfile

import pytest

import gen

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_CHECKSUM, E_NOENT = 0, -1, -4, -5, -7, -9
POM = "META-INF/maven/g/a/pom.xml"


def pom_text(i):
    n = 1024 + (i * 997) % (7 * 1024)                      # 1 .. 8 KiB
    body = b"".join(b"<dependency><groupId>g%d</groupId><artifactId>a%d</artifactId><version>%d.%d</version></dependency>\n" % (k, i, k % 7, i % 11)
                    for k in range(200))
    return (b"<project><modelVersion>4.0.0</modelVersion><artifactId>jar%d</artifactId>\n" % i + body)[:n - 11] + b"</project>\n"


def make_jar(i, pom=True, big=False):
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        zf.writestr(zipfile.ZipInfo("META-INF/MANIFEST.MF"), b"Manifest-Version: 1.0\nCreated-By: test %d\n" % i, zipfile.ZIP_STORED)
        for k in range(1 + i % 3):
            zf.writestr(zipfile.ZipInfo(f"g/a/C{k}.class"), b"\xca\xfe\xba\xbe" + gen.pseudo_text(700 + 111 * k, seed=i + k), zipfile.ZIP_DEFLATED if (i + k) % 2 else zipfile.ZIP_STORED)
        if big:
            for k in range(3):                                # more than 8 MiB in front of the pom
                zf.writestr(zipfile.ZipInfo(f"g/a/blob{k}.bin"), gen.incompressible(40 + k, 3 << 20), zipfile.ZIP_STORED)
        if pom and not big:
            zf.writestr(zipfile.ZipInfo(POM), pom_text(i), zipfile.ZIP_STORED if i % 5 == 0 else zipfile.ZIP_DEFLATED)
            zf.writestr(zipfile.ZipInfo("META-INF/maven/g/a/pom.properties"), b"version=1.%d\n" % i, zipfile.ZIP_STORED)
        if big:
            zf.writestr(zipfile.ZipInfo(POM), pom_text(i), zipfile.ZIP_DEFLATED)          # its pom last
        if i % 7 == 0:
            zf.comment = b"built for the test " * (i % 4 + 1)
    return b.getvalue()


@pytest.fixture(scope="module")
def jars():
    files = {f"repo/g/a/{i}/a-{i}.jar": make_jar(i) for i in range(40)}
    files["repo/nopom.jar"] = make_jar(100, pom=False)
    files["repo/text.jar"] = gen.text(3000)
    files["repo/big.jar"] = make_jar(200, big=True)
    assert len(files["repo/big.jar"]) > 9 << 20
    return files


@pytest.fixture(scope="module")
def archives(jars, tmp_path_factory):
    """no_skip -> (open archive, its path, its index rows), written on first use"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    d = tmp_path_factory.mktemp("zip_entries")
    for k, v in jars.items():
        (d / "in" / k).parent.mkdir(parents=True, exist_ok=True)
        (d / "in" / k).write_bytes(v)
    made = {}

    def get(no_skip):
        if no_skip not in made:
            p = d / f"a{int(no_skip)}.znippy"
            host.compress_dir(d / "in", p, no_skip)
            rows = host.read_index(p)[0]
            assert any(r["compressed"] for r in rows if r["relative_path"].endswith(".jar")) == no_skip
            assert sum(1 for r in rows if r["relative_path"] == "repo/big.jar") >= 2                  # the big jar spans chunks
            made[no_skip] = (host.ZnippyArchive.open(p), p, rows)
        return made[no_skip]
    yield get
    for a, _, _ in made.values():
        a.close()


@pytest.fixture(scope="module", params=[False, True], ids=["stored", "no_skip"])
def archive(request, archives):
    return archives(request.param)


def expected(jars, path):
    if path not in jars:
        return E_INVAL, None
    try:
        zf = zipfile.ZipFile(io.BytesIO(jars[path]))
    except zipfile.BadZipFile:
        return E_CORRUPT, None
    names = [n for n in zf.namelist() if n.endswith("pom.xml")]
    return (OK, zf.read(names[0])) if names else (E_NOENT, None)


def test_every_pom_in_one_batch(archive, jars):
    a, _, _ = archive
    paths = sorted(jars) + ["repo/unknown.jar"]
    got, st = a.extract_zip_entries(paths, "pom.xml")
    for p, g, s in zip(paths, got, st):
        want_st, want = expected(jars, p)
        assert s == want_st, (p, s, want_st)
        assert g == want, p
    assert st.count(OK) == 41 and st[paths.index("repo/nopom.jar")] == E_NOENT and st[paths.index("repo/text.jar")] == E_CORRUPT and st[-1] == E_INVAL
    # prefix and suffix together; a filter that matches the first entry of every jar; one that matches nothing
    got, st = a.extract_zip_entries(paths[:5], ".xml", prefix="META-INF/maven/")
    assert [g for g in got] == [expected(jars, p)[1] for p in paths[:5]]
    got, st = a.extract_zip_entries(["repo/g/a/3/a-3.jar", "repo/big.jar"], "", prefix="META-INF/MANIFEST")
    assert st == [OK, OK] and got[0].startswith(b"Manifest-Version") and got[1].endswith(b"test 200\n")
    got, st = a.extract_zip_entries(paths[:3], ".nothing")
    assert st == [E_NOENT] * 3 and got == [None] * 3
    assert a.extract_zip_entries([], "pom.xml") == ([], [])


def test_cap_one_byte_short(archive, jars):
    a, _, _ = archive
    paths = [p for p in sorted(jars) if expected(jars, p)[0] == OK][:6]
    sizes = [len(expected(jars, p)[1]) for p in paths]
    got, st = a.extract_zip_entries(paths, "pom.xml", cap=sum(sizes))
    assert st == [OK] * 6
    got, st = a.extract_zip_entries(paths, "pom.xml", cap=sum(sizes) - 1)
    assert st == [OK] * 5 + [E_DST_SMALL] and got[5] is None
    assert got[:5] == [expected(jars, p)[1] for p in paths[:5]]
    # a file in the middle that does not fit leaves the ones in front of it clean
    got, st = a.extract_zip_entries(paths, "pom.xml", cap=sum(sizes[:3]) - 1)
    assert st[:2] == [OK, OK] and st[2] == E_DST_SMALL and got[:2] == [expected(jars, p)[1] for p in paths[:2]]


def test_a_flipped_byte_of_one_pom(archives, jars, tmp_path):
    from znippy_amd import host
    _, p, rows = archives(False)                         # jars stored: the archive file holds the jar's own bytes
    victim = "repo/g/a/3/a-3.jar"                        # a deflated pom
    (row,) = [r for r in rows if r["relative_path"] == victim]
    assert not row["compressed"]
    zf = zipfile.ZipFile(io.BytesIO(jars[victim]))
    zi = zf.getinfo(POM)
    assert zi.compress_type == zipfile.ZIP_DEFLATED
    at = row["blob_offset"] + zi.header_offset + 30 + len(zi.filename) + zi.compress_size // 2
    q = tmp_path / "damaged.znippy"
    shutil.copyfile(p, q)
    raw = bytearray(q.read_bytes())
    assert bytes(raw[row["blob_offset"]:row["blob_offset"] + len(jars[victim])]) == jars[victim]     # a stored row is the jar
    raw[at] ^= 0x10
    q.write_bytes(bytes(raw))
    a = host.ZnippyArchive.open(q)
    paths = ["repo/g/a/2/a-2.jar", victim, "repo/g/a/4/a-4.jar"]
    got, st = a.extract_zip_entries(paths, "pom.xml")
    a.close()
    assert st[0] == OK and st[2] == OK and st[1] in (E_CHECKSUM, E_CORRUPT), st
    assert got[0] == expected(jars, paths[0])[1] and got[2] == expected(jars, paths[2])[1] and got[1] is None
