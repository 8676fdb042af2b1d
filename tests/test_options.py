"""The MB_* options: one table (csrc/mb_options.h), every read through it, and what mb_set_option / mb_get_option do with it.

Host code only: nothing here needs a device.  The list of options lives in the table alone -- the tests take it from
`capi.options()` (mb_get_option(NULL)) and never spell it out.
"""
import os
import re

import pytest

from randmachine import random_machine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "machineboss_amd", "csrc")
TABLE_FILES = ("mb_options.h", "mb_options.cpp")
OLD_READERS = ("env_int", "env_int_early", "env_int_m", "env_int_w", "env_int_s", "env_int_g", "jenv", "env_flag_default", "opt_env")
UNKNOWN = "MB_WIDE_LANEZ"      # a misspelt MB_WIDE_LANES


def _sources(strip_comments):
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f in TABLE_FILES or not f.endswith((".h", ".hip", ".cpp")):
            continue
        text = open(os.path.join(CSRC, f)).read()
        if strip_comments:
            text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
            text = re.sub(r"//[^\n]*", " ", text)
        out[f] = text
    return out


@pytest.fixture(scope="module")
def capi():
    from machineboss_amd import capi
    return capi


@pytest.fixture(scope="module")
def table(capi):
    return capi.options()


@pytest.fixture()
def tiny():
    return random_machine(25, 0, 3, 5, density=1.5, silent_density=1.0, allow_inf=False)      # one tape, below 192 states: 256 lanes by default


def _get(capi, name):
    v = capi.load().mb_get_option(None if name is None else name.encode())
    return None if v is None else v.decode()


def test_no_stray_names_in_the_sources(table):
    code = _sources(strip_comments=True)
    for f, text in code.items():
        assert re.findall(r'"MB_[A-Z0-9_]*"', text) == [], f
    everything = "\n".join(code.values())
    unused = [name for name in table if not re.search(r"\b%s\b" % name, everything)]
    assert unused == []
    for f, text in _sources(strip_comments=False).items():      # (comments included: the old readers are gone by name too)
        assert re.findall(r"\b(?:%s)\b" % "|".join(OLD_READERS), text) == [], f


def test_the_table_is_complete(table, capi):
    """128 entries: the names that

        git grep -ohE '"MB_[A-Z0-9_]*"' <parent commit> -- machineboss_amd/csrc | sort -u | grep -v '^"MB_"$'

    harvests from the commit before the table (129 distinct literals, one of them the bare "MB_" prefix that mb_set_option
    compared names with -- no option).  With test_no_stray_names_in_the_sources (every entry is read somewhere, no name is read
    outside the table) the count pins the set."""
    assert len(table) == 128
    assert len(_get(capi, None).splitlines()) == 128      # (no name twice)
    for name, e in table.items():
        assert re.fullmatch(r"MB_[A-Z0-9_]+", name)
        assert e["kind"] in ("Int", "Real", "Text", "Present") and e["class"] in ("host", "planner", "diagnostic", "experiment", "info")
        assert e["note"]
        if e["kind"] in ("Text", "Present") or e["class"] == "info":
            assert e["default"] == "-"
        else:
            assert e["default"] == "by call" or re.fullmatch(r"-?[0-9.]+", e["default"])
    assert sorted(n for n, e in table.items() if e["class"] == "experiment") == ["MB_JIT_DEBUG", "MB_WIDE_JIT_KNOCKOUT"]
    assert [n for n, e in table.items() if e["class"] == "info"] == ["MB_INFO_INPLACE_RING_KERNELS"]
    assert table["MB_WIDE_LANES"]["default"] == "by call"
    assert (table["MB_ONETAPE_PART_TIMEOUT_S"]["kind"], table["MB_ONETAPE_PART_TIMEOUT_S"]["default"]) == ("Real", "20")
    assert table["MB_MEDIUM_PERSIST_TIMEOUT_S"]["default"] == "20" and table["MB_SMALL_ONE_LAUNCH_TIMEOUT_S"]["default"] == "20"


def test_set_option_semantics(capi, monkeypatch):
    L = capi.load()
    name = "MB_MEDIUM_STREAMS"
    monkeypatch.delenv(name, raising=False)
    try:
        assert _get(capi, name) is None
        capi.set_option(name, 3)
        assert _get(capi, name) == "3"                       # set, then get
        monkeypatch.setenv(name, "1")
        assert _get(capi, name) == "3"                       # the override wins over the environment
        capi.set_option(name, None)
        assert _get(capi, name) == "1"                       # NULL: the environment's value again
        capi.set_option(name, 4)
        capi.set_option(name, "")
        assert _get(capi, name) == "1"                       # "": the same
        monkeypatch.delenv(name)
        assert _get(capi, name) is None
        # a name that is not in the table: refused, named, nothing changes
        before = _get(capi, None)
        assert L.mb_set_option(UNKNOWN.encode(), b"512") != 0
        assert "unknown option" in L.mb_last_error().decode() and UNKNOWN in L.mb_last_error().decode()
        with pytest.raises(capi.MbError, match=UNKNOWN):
            capi.set_option(UNKNOWN, 512)
        assert L.mb_set_option(b"WIDE_LANES", b"512") != 0 and L.mb_set_option(b"", b"1") != 0 and L.mb_set_option(None, b"1") != 0
        assert L.mb_set_option(UNKNOWN.encode(), None) != 0      # (also when it would only remove)
        assert _get(capi, UNKNOWN) is None and _get(capi, "") is None and _get(capi, "MB_") is None
        assert _get(capi, None) == before and _get(capi, "MB_WIDE_LANES") is None
        # the read-only entry
        info = "MB_INFO_INPLACE_RING_KERNELS"
        assert int(_get(capi, info)) >= 0
        assert L.mb_set_option(info.encode(), b"7") != 0 and info in L.mb_last_error().decode()
        assert int(_get(capi, info)) >= 0 and _get(capi, info) != "7"
    finally:
        capi.set_option(name, None)


def test_nothing_is_cached(capi, tiny, monkeypatch, tmp_path):
    lanes = lambda: capi.debug_wide_retimed(tiny, str(tmp_path / "p.bin"), capi.MB_VITERBI, False)["lanes"]
    monkeypatch.delenv("MB_WIDE_LANES", raising=False)
    try:
        assert lanes() == 256
        monkeypatch.setenv("MB_WIDE_LANES", "512")
        assert lanes() == 512
        monkeypatch.setenv("MB_WIDE_LANES", "")              # empty: an Int takes its default
        assert lanes() == 256
        monkeypatch.delenv("MB_WIDE_LANES")
        assert lanes() == 256
        capi.set_option("MB_WIDE_LANES", 512)
        assert lanes() == 512
        monkeypatch.setenv("MB_WIDE_LANES", "128")
        assert lanes() == 512                                # (the override wins)
        capi.set_option("MB_WIDE_LANES", None)
        assert lanes() == 128
    finally:
        capi.set_option("MB_WIDE_LANES", None)


def test_present_kind(capi, table, tiny, monkeypatch, tmp_path, capfd):
    assert table["MB_WIDE_VERBOSE"]["kind"] == "Present"
    def log():
        capfd.readouterr()
        capi.debug_wide_retimed(tiny, str(tmp_path / "p.bin"), capi.MB_VITERBI, False)
        return capfd.readouterr().err
    monkeypatch.delenv("MB_WIDE_VERBOSE", raising=False)
    try:
        assert "[mbhip]" not in log()
        monkeypatch.setenv("MB_WIDE_VERBOSE", "")            # an empty environment value counts as set
        assert _get(capi, "MB_WIDE_VERBOSE") == "" and "[mbhip]" in log()
        monkeypatch.delenv("MB_WIDE_VERBOSE")
        capi.set_option("MB_WIDE_VERBOSE", "0")              # any value does
        assert "[mbhip]" in log()
        capi.set_option("MB_WIDE_VERBOSE", "")               # through mb_set_option "" removes the override: unset
        assert _get(capi, "MB_WIDE_VERBOSE") is None and "[mbhip]" not in log()
    finally:
        capi.set_option("MB_WIDE_VERBOSE", None)


def test_design_section_lists_the_host_entries(table):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^### 4\.7 [^\n]*\n(.*?)^## ", text, flags=re.S | re.M)
    assert m
    rows = set(re.findall(r"\bMB_[A-Z0-9_]+\b", m.group(1)))
    assert rows == {name for name, e in table.items() if e["class"] == "host"}
