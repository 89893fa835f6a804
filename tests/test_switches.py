"""The library's environment switches are stated once, in graphtyper_amd/csrc/gtx_switches.hpp: no other file of the library asks the
environment, the host emulations read the library's switches through that header, README.md's switch paragraph names exactly the
header's table (plus the variables the Python side reads), the names that were retired stay away, and the readers' value rules --
run as a stand-alone program under AddressSanitizer / UBSan (tests/emu_switches) -- are the ones written out below."""
import functools
import glob
import os
import re

import pytest

import emu_programs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graphtyper_amd", "csrc")
HEADER = os.path.join(CSRC, "gtx_switches.hpp")
SOURCE = (".cpp", ".hpp", ".hip", ".inl", ".h", ".mk", ".py")


def read(path):
    with open(path, errors="replace") as f:
        return f.read()


def sources(*dirs):
    for d in dirs:
        for base, _, names in os.walk(d):
            for n in names:
                if n.endswith(SOURCE) or n == "Makefile":
                    yield os.path.join(base, n)


def emu_dirs():
    return sorted(d for d in glob.glob(os.path.join(HERE, "emu*")) if os.path.isdir(d))


def table():
    """the names of the header's table: the comment lines in front of `#pragma once` that begin with a name"""
    head = read(HEADER).split("#pragma once")[0]
    return re.findall(r"^//   (GTX_[A-Z0-9_]+) ", head, flags=re.M)


def python_side():
    """what bench.py and the package read from os.environ"""
    names = set()
    for path in [os.path.join(ROOT, "bench.py")] + glob.glob(os.path.join(ROOT, "graphtyper_amd", "*.py")):
        names.update(re.findall(r"""environ(?:\.get|\.setdefault)?[\[(]\s*["'](GTX_[A-Z0-9_]+)["']""", read(path)))
    return names


def switch_paragraph():
    text = read(os.path.join(ROOT, "README.md"))
    at = text.index("\nSwitches read from the environment")
    return text[at + 1:].split("\n\n")[0]


def test_only_the_header_asks_the_environment():
    asking = sorted(os.path.relpath(p, CSRC) for p in sources(CSRC) if "getenv" in read(p))
    assert asking == ["gtx_switches.hpp"]


def test_the_emulations_ask_for_their_own_variables_only():
    assert len(emu_dirs()) >= 2
    for path in sources(*emu_dirs()):
        text = read(path)
        own = re.findall(r"""getenv\("GTX_EMU_[A-Z0-9_]+"\)""", text)
        assert len(own) == text.count("getenv"), os.path.relpath(path, ROOT)


def test_the_table_has_every_reader_s_name():
    """a name between quotes in the header's code is a line of its table, and the other way round"""
    code = read(HEADER).split("#pragma once")[1]
    names = table()
    assert len(names) == len(set(names)) and set(names) == set(re.findall(r'"(GTX_[A-Z0-9_]+)"', code))


def test_readme_names_the_table():
    paragraph = set(re.findall(r"GTX_[A-Z0-9_]+", switch_paragraph()))
    assert set(table()) - paragraph == set()
    assert paragraph - set(table()) - python_side() == set()


# what section B of the change retired: environment switches nothing set, build macros nothing defined
RETIRED = ["GTX_INDEX_BUILD", "GTX_FILTER_BITS_LOG2", "GTX_EXACT_LARGE_PARTS", "GTX_SKIP_HBM_PASSES", "GTX_EXPERIMENT", "GTX_SCORE_ADDS_CALLED",
           "GTX_SCORE_ADD_INLINE", "GTX_NO_WAVE_GROUP", "GTX_NO_NT", "GTX_SCORE_WAVES", "GTX_SCORE_ATTR", "GTX_NO_SCORE_STAGING", "GTX_HINT_REC_SLOT",
           "GTX_NO_NEAR_FREE", "GTX_PROF_SCORE", "GTX_PS", "GTX_HARD_SYNC", "GTX_EXACT_PASS_WAVES", r"GTX_X_[A-Z0-9_]+"]
# ... and two whose build constant stays in the code: gone as environment variables (a name between quotes) and from the documents
RETIRED_READS = ["GTX_EXACT_PARTS_MAX", "GTX_BIG_BLOCKS_PER_CU"]


def whole(name):
    """the name as a word of its own, behind a compiler's -D too"""
    return re.compile(r"(?:(?<![A-Za-z0-9_])|(?<=-D))%s(?![A-Za-z0-9_])" % name)


def test_the_retired_names_are_gone():
    documents = [os.path.join(ROOT, "README.md"), os.path.join(ROOT, "DESIGN.md")]
    found = []
    for path in list(sources(CSRC, *emu_dirs())) + documents:
        text = read(path)
        found += [(os.path.relpath(path, ROOT), m.group(0)) for name in RETIRED for m in whole(name).finditer(text)]
        found += [(os.path.relpath(path, ROOT), name) for name in RETIRED_READS if ('"%s"' % name) in text or (path in documents and whole(name).search(text))]
    assert found == []


# ---- the readers' value rules: the program's line for a setting is the line of an empty environment with these words changed.
# Every value is what the code in front of the header did with the setting (the library's parse where the emulation's differed).
CAP = int(re.search(r"\bHALF_BUCKET_CAP = (\d+);", read(os.path.join(CSRC, "graph_dev.hpp"))).group(1))
UNSET = dict(force=0, four=1, hinted=1, decline_all=0, wide="01", hint_dense="01", hint_less=0, hint_more=1, nb_known=1, index_runs=1, build_stream=1,
             big_grid_adaptive=1, bgzf_crc=1, timing=0, host_threads=0, half_bucket_cap=CAP, hint_windows=16384, device_cache_mb=32768, time_every=1,
             bgzf_threads=16, bgzf_linger_us=300, bgzf_device_ring=256, bgzf_device=0, inflate_zlib=0, exact_pass_mb=0, exact_parts=0)
NO_PASS_0 = dict(hinted=0)
CASES = [
    ({}, {}),
    # pass 1: 0 = one read per wavefront, and no pass 0 with it; l... / w... force a build (both graph choices give it)
    ({"GTX_EXPRESS4": ""}, {}),
    ({"GTX_EXPRESS4": "0"}, dict(four=0, hinted=0)),
    ({"GTX_EXPRESS4": "1"}, {}),
    ({"GTX_EXPRESS4": "lean"}, dict(wide="00")),
    ({"GTX_EXPRESS4": "l"}, dict(wide="00")),
    ({"GTX_EXPRESS4": "wide"}, dict(wide="11")),
    ({"GTX_EXPRESS4": "w"}, dict(wide="11")),
    # pass 0
    ({"GTX_HINT": "0"}, NO_PASS_0),
    ({"GTX_HINT": "d"}, dict(decline_all=1)),
    ({"GTX_HINT": "decline"}, dict(decline_all=1)),
    ({"GTX_HINT": "1"}, {}),
    ({"GTX_HINT": "1", "GTX_EXPRESS4": "0"}, dict(four=0, hinted=0)),
    ({"GTX_HINT": "d", "GTX_EXPRESS4": "0"}, dict(four=0, hinted=0)),
    ({"GTX_HINT_BUILD": "lean"}, dict(hint_dense="00")),
    ({"GTX_HINT_BUILD": "dense"}, dict(hint_dense="11")),
    ({"GTX_HINT_BUILD": "x"}, {}),
    ({"GTX_HINT_BUILD": "dense", "GTX_HINT": "0"}, NO_PASS_0),  # (not looked at without the pass)
    ({"GTX_HINT_MORE": "0"}, dict(hint_more=0, hint_less=1)),
    ({"GTX_HINT_MORE": "1"}, {}),
    ({"GTX_HINT_MORE": "0", "GTX_HINT": "0"}, dict(hint_more=0, hinted=0)),
    # 1 = through all passes, any other number but 0 counts as 2; both make pass 0 decline everything
    ({"GTX_FORCE_SECOND_PASS": "0"}, {}),
    ({"GTX_FORCE_SECOND_PASS": "1"}, dict(force=1, decline_all=1)),
    ({"GTX_FORCE_SECOND_PASS": "2"}, dict(force=2, decline_all=1)),
    ({"GTX_FORCE_SECOND_PASS": "x"}, {}),
    ({"GTX_FORCE_SECOND_PASS": "3"}, dict(force=2, decline_all=1)),
    ({"GTX_FORCE_SECOND_PASS": "-1"}, dict(force=2, decline_all=1)),
    ({"GTX_FORCE_SECOND_PASS": "1", "GTX_HINT": "0"}, dict(force=1, hinted=0)),
    # the exact pass: the value, or 0 = not given
    ({"GTX_EXACT_PARTS": "0"}, {}),
    ({"GTX_EXACT_PARTS": "-3"}, {}),
    ({"GTX_EXACT_PARTS": "64"}, dict(exact_parts=64)),
    ({"GTX_EXACT_PARTS": "5000"}, dict(exact_parts=1024)),
    ({"GTX_EXACT_PASS_MB": "0"}, {}),
    ({"GTX_EXACT_PASS_MB": "-1"}, {}),
    ({"GTX_EXACT_PASS_MB": "x"}, {}),
    ({"GTX_EXACT_PASS_MB": "512"}, dict(exact_pass_mb=512)),
    # numbers, clamped; what is no number counts as 0
    ({"GTX_HALF_BUCKET_CAP": "-1"}, dict(half_bucket_cap=0)),
    ({"GTX_HALF_BUCKET_CAP": "0"}, dict(half_bucket_cap=0)),
    ({"GTX_HALF_BUCKET_CAP": "1"}, dict(half_bucket_cap=1)),
    ({"GTX_HALF_BUCKET_CAP": str(CAP + 1)}, {}),
    ({"GTX_HALF_BUCKET_CAP": "x"}, dict(half_bucket_cap=0)),
    ({"GTX_HINT_WINDOWS": "0"}, dict(hint_windows=0)),
    ({"GTX_HINT_WINDOWS": "-5"}, dict(hint_windows=0)),
    ({"GTX_HINT_WINDOWS": "100"}, dict(hint_windows=100)),
    ({"GTX_DEVICE_CACHE_MB": "-1"}, dict(device_cache_mb=0)),
    ({"GTX_DEVICE_CACHE_MB": "0"}, dict(device_cache_mb=0)),
    ({"GTX_DEVICE_CACHE_MB": "1024"}, dict(device_cache_mb=1024)),
    ({"GTX_HOST_THREADS": "4"}, dict(host_threads=4)),
    ({"GTX_HOST_THREADS": "0"}, dict(host_threads=1)),
    ({"GTX_HOST_THREADS": "-2"}, dict(host_threads=1)),
    ({"GTX_HOST_THREADS": "x"}, dict(host_threads=1)),
    ({"GTX_TIME_EVERY": "4"}, dict(time_every=4)),
    ({"GTX_TIME_EVERY": "0"}, {}),
    ({"GTX_TIME_EVERY": "-1"}, {}),
    ({"GTX_BGZF_THREADS": "0"}, dict(bgzf_threads=0)),
    ({"GTX_BGZF_THREADS": "-1"}, dict(bgzf_threads=0)),
    ({"GTX_BGZF_THREADS": "3"}, dict(bgzf_threads=3)),
    ({"GTX_BGZF_LINGER_US": "0"}, dict(bgzf_linger_us=0)),
    ({"GTX_BGZF_LINGER_US": "-5"}, dict(bgzf_linger_us=0)),
    ({"GTX_BGZF_LINGER_US": "50"}, dict(bgzf_linger_us=50)),
    ({"GTX_BGZF_DEVICE_RING": "1"}, dict(bgzf_device_ring=32)),
    ({"GTX_BGZF_DEVICE_RING": "1000"}, dict(bgzf_device_ring=1000)),
    ({"GTX_BGZF_DEVICE_RING": "100000"}, dict(bgzf_device_ring=65536)),
    # on for anything but nothing and the one character 0
    ({"GTX_BGZF_DEVICE": ""}, {}),
    ({"GTX_BGZF_DEVICE": "0"}, {}),
    ({"GTX_BGZF_DEVICE": "1"}, dict(bgzf_device=1)),
    ({"GTX_BGZF_DEVICE": "00"}, dict(bgzf_device=1)),
    ({"GTX_INFLATE": "zlib"}, dict(inflate_zlib=1)),
    ({"GTX_INFLATE": "own"}, {}),
    ({"GTX_INFLATE": ""}, {}),
    # set to anything
    ({"GTX_TIMING": ""}, dict(timing=1)),
    ({"GTX_TIMING": "0"}, dict(timing=1)),
]
# off when the value starts with 0
for _name, _word in [("GTX_NB_KNOWN", "nb_known"), ("GTX_INDEX_RUNS", "index_runs"), ("GTX_BUILD_STREAM", "build_stream"),
                     ("GTX_BIG_GRID_ADAPTIVE", "big_grid_adaptive"), ("GTX_BGZF_CRC", "bgzf_crc")]:
    CASES += [({_name: "0"}, {_word: 0}), ({_name: "00"}, {_word: 0}), ({_name: "1"}, {}), ({_name: ""}, {})]


@pytest.fixture(scope="session")
def program(tmp_path_factory):
    return emu_programs.build("emu_switches", tmp_path_factory.mktemp("emu_switches"))


def test_the_cases_cover_the_table():
    assert {name for setting, _ in CASES for name in setting} == set(table())


def test_the_readers_rules(program, tmp_path):
    """every setting of CASES in one run of the program (no sanitizer report, or emu_programs.Died): set, ask, unset"""
    def write(path):
        with open(path, "w") as f:
            f.write("".join("-%s\n" % name for name in table()))  # (whatever this process inherited or set: bench.py, once imported, sets one)
            for setting, _ in CASES:
                f.write("".join("%s=%s\n" % kv for kv in setting.items()) + "?\n" + "".join("-%s\n" % k for k in setting))

    def parse(path):
        return [dict(word.split("=") for word in line.split()) for line in read(path).splitlines()]
    got = functools.partial(emu_programs.run, program, tmp_path)(write, parse)
    assert len(got) == len(CASES)
    wrong = []
    for (setting, change), line in zip(CASES, got):
        want = {k: str(v) for k, v in dict(UNSET, **change).items()}
        if line != want:
            wrong.append((setting, {k: (line.get(k), want.get(k)) for k in set(line) | set(want) if line.get(k) != want.get(k)}))
    assert wrong == []
