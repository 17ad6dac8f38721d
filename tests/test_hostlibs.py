"""tests/hostlibs.py: the build table of the native test libraries and the defaults of their front ends.  Nothing here compiles or loads a library."""
import os
import re

import pytest

import hostlibs

FRONT_ENDS = ("helpers.py", "path_sedge_helpers.py", "path_guide_helpers.py", "collocated_helpers.py", "smooth_cases.py")


def _includes(path, seen):
    """every file `path` pulls in through #include "...", transitively (resolved against the including file, as the compiler does first)"""
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        f = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        assert os.path.exists(f), "%s includes %s, which is not there" % (path, inc)
        if f not in seen:
            seen.add(f)
            _includes(f, seen)
    return seen


@pytest.mark.parametrize("name", sorted(hostlibs.LIBS))
def test_a_library_is_stale_against_everything_its_source_includes(name):
    """an edit to any header a harness includes -- psdr_reverse.h through psdr_path_sedge.h, say -- must rebuild it: the lazy loader once went by a hand-written
    list that had forgotten the adjoints"""
    deps = set(hostlibs.deps(name))
    src = hostlibs.source(name)
    assert src in deps and os.path.exists(src)
    missing = _includes(src, set()) - deps
    assert not missing, "%s: not in the dependency set: %s" % (name, sorted(missing))
    if "hostcheck" in hostlibs.LIBS[name][0] and name != "smooth":
        assert os.path.join(hostlibs.CSRC, "psdr_reverse.h") in deps and os.path.join(hostlibs.HC_DIR, "host_common.h") in deps


def test_the_default_thread_count_is_capped(monkeypatch):
    assert 1 <= hostlibs.host_threads() <= 16
    for cpus, want in ((192, 16), (16, 16), (3, 3), (None, 1)):
        monkeypatch.setattr(os, "cpu_count", lambda c=cpus: c)
        assert hostlibs.host_threads() == want
    # no front end sizes a thread pool by the machine: a command on the GPU machines has 16 CPUs of several times as many
    for f in FRONT_ENDS:
        assert "cpu_count" not in open(os.path.join(hostlibs.TESTS, f)).read(), f
