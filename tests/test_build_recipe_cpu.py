"""The build recipe's one compile-and-link function (build.compile_and_link) on two trivial sources in a temporary directory, with
the real compiler and the real FLAGS: which sources a call recompiles, and whether it relinks.  Every case first brings
the tree up to date with the plain command, so the cases do not depend on their order."""
import json
import os
import shutil

import pytest

from tissue_analysis_amd import build

ROOT = os.path.realpath(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


FILES = {"x.h": "#define X 1\n", "y.h": "#define Y 2\n",
         "a.hip": '#include "x.h"\nextern "C" int fa() { return X; }\n',
         "b.hip": '#include "y.h"\nextern "C" int fb() { return Y; }\n'}


class Tree:
    def __init__(self, root):
        self.src, self.obj, self.lib = os.path.join(root, "src"), os.path.join(root, "obj"), os.path.join(root, "libab.so")
        os.makedirs(self.src)
        for name, text in FILES.items():
            self.write(name, text)

    def path(self, name):
        return os.path.join(self.obj if name.endswith((".o", ".json")) else self.src, name)

    def write(self, name, text):
        with open(self.path(name), "w") as f:
            f.write(text)

    def build(self, **kw):
        return build.compile_and_link(self.src, ["a.hip", "b.hip"], self.obj, self.lib, build.FLAGS, **kw)

    def touch(self, name):
        """Make `name` a millisecond newer than everything built so far: no waiting for the clock, and what a compile
        writes next (it takes a second) is newer again."""
        t = max(os.stat(p).st_mtime_ns for p in (self.path("a.o"), self.path("b.o"), self.lib)) + 1000000
        os.utime(self.path(name), ns=(t, t))

    def lib_stamp(self):
        return os.stat(self.lib).st_mtime_ns


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    tree = Tree(str(tmp_path_factory.mktemp("recipe")))
    return tree, tree.build()


@pytest.fixture
def tree(first):
    """The tree as the plain command leaves it, whatever the case before did to it."""
    t = first[0]
    for name, text in FILES.items():
        if not os.path.exists(t.path(name)) or open(t.path(name)).read() != text:
            t.write(name, text)
    t.build()
    assert t.build() == []
    return t


def test_first_call_compiles_both_and_links(first):
    tree, compiled = first
    assert compiled == ["a.hip", "b.hip"]
    assert os.path.exists(tree.lib) and os.path.exists(tree.path("a.o")) and os.path.exists(tree.path("b.o"))
    rec = json.load(open(tree.path("a.o.json")))
    assert rec["deps"] == ["a.hip", "x.h"] and os.path.isabs(rec["argv"][0]) and "version" in rec["compiler"]
    assert rec["argv"][1:] == build.FLAGS + ["-c", tree.path("a.hip"), "-o", tree.path("a.o")]
    assert json.load(open(tree.path("b.o.json")))["deps"] == ["b.hip", "y.h"]


def test_second_call_compiles_nothing_and_does_not_relink(tree):
    stamp = tree.lib_stamp()
    assert tree.build() == []
    assert tree.lib_stamp() == stamp


def test_a_touched_header_recompiles_its_includer_only(tree):
    tree.touch("x.h")
    stamp = tree.lib_stamp()
    assert tree.build() == ["a.hip"]
    assert tree.lib_stamp() != stamp
    assert tree.build() == []


def test_a_touched_source_recompiles_itself_only(tree):
    tree.touch("a.hip")
    assert tree.build() == ["a.hip"]


def test_a_define_recompiles_both_once(tree):
    assert tree.build(defines=["-DEXTRA=1"]) == ["a.hip", "b.hip"]
    assert "-DEXTRA=1" in json.load(open(tree.path("b.o.json")))["argv"]
    stamp = tree.lib_stamp()
    assert tree.build(defines=["-DEXTRA=1"]) == []
    assert tree.lib_stamp() == stamp


def test_a_per_source_flag_recompiles_that_source_only(tree):
    assert tree.build(extra_flags={"b.hip": ["-ffp-contract=off"]}) == ["b.hip"]
    assert tree.build(extra_flags={"b.hip": ["-ffp-contract=off"]}) == []


def test_a_deleted_object_is_recompiled(tree):
    os.remove(tree.path("b.o"))
    assert tree.build() == ["b.hip"]


def test_a_deleted_record_recompiles_its_source(tree):
    os.remove(tree.path("a.o.json"))
    assert tree.build() == ["a.hip"]
    os.remove(tree.path("libab.so.json"))
    stamp = tree.lib_stamp()
    assert tree.build() == []
    assert tree.lib_stamp() != stamp          # (no record of the link: it runs again)


def test_a_dependency_that_is_gone_recompiles_and_builds(tree):
    tree.write("z.h", "#define Z 3\n")
    tree.write("b.hip", '#include "y.h"\n#include "z.h"\nextern "C" int fb() { return Y + Z; }\n')
    tree.touch("b.hip")
    assert tree.build() == ["b.hip"]
    assert json.load(open(tree.path("b.o.json")))["deps"] == ["b.hip", "y.h", "z.h"]
    os.remove(tree.path("z.h"))
    tree.write("b.hip", FILES["b.hip"])
    os.utime(tree.path("b.hip"), (0, 0))      # (older than the object: only the missing header makes it stale)
    assert tree.build() == ["b.hip"]
    assert json.load(open(tree.path("b.o.json")))["deps"] == ["b.hip", "y.h"]


def test_a_failed_compile_is_not_skipped_by_the_next_call(tree, capfd):
    tree.write("a.hip", '#include "x.h"\nextern "C" int fa() { return X +; }\n')
    tree.touch("a.hip")
    with pytest.raises(RuntimeError):
        tree.build()
    assert "a.hip" in capfd.readouterr().err
    assert not os.path.exists(tree.path("a.o.json"))
    tree.write("a.hip", FILES["a.hip"])
    os.utime(tree.path("a.hip"), (0, 0))      # (older than any object the failed compile may have left)
    assert tree.build() == ["a.hip"]


def test_a_library_without_its_objects_is_a_full_build(tree):
    shutil.rmtree(tree.obj)
    assert os.path.exists(tree.lib)
    assert tree.build() == ["a.hip", "b.hip"]


def test_force_compiles_both(tree):
    assert tree.build(force=True) == ["a.hip", "b.hip"]


def test_one_job_builds_the_same_objects(tree, monkeypatch):
    monkeypatch.setenv("MAX_JOBS", "16")
    assert tree.build(force=True) == ["a.hip", "b.hip"]
    parallel = [open(tree.path(o), "rb").read() for o in ("a.o", "b.o")]
    monkeypatch.setenv("MAX_JOBS", "1")
    assert build._jobs() == 1
    assert tree.build(force=True) == ["a.hip", "b.hip"]
    assert [open(tree.path(o), "rb").read() for o in ("a.o", "b.o")] == parallel
    monkeypatch.setenv("MAX_JOBS", "64")
    assert build._jobs() == 16


def test_sources_are_the_hip_files_of_csrc():
    assert build.SOURCES == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert len(set(build.SOURCES)) == len(build.SOURCES) > 0
    assert not hasattr(build, "HEADERS")


def test_every_product_source_has_a_record_after_build():
    build.build()
    for src in build.SOURCES:
        deps = build.dependencies(src)
        assert deps[0] == src, deps
        for d in deps:
            full = os.path.realpath(os.path.join(build.CSRC, d))
            assert full.startswith(ROOT + os.sep) and os.path.exists(full), (src, d)
    assert "ta_ctx.h" in build.dependencies("ta_api.hip")
