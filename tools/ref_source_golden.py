#!/usr/bin/env python3
"""Facts the tests take from the reference's SOURCES rather than from its compiled library, kept as fixtures under
tests/golden/ so that the tests hold where the sources are not (build container only to regenerate):

  ref_tables.json           the constant tables of the reference's DSP code, as its source text spells them
                            (tests/test_oracle_tables.py)
  ref_vtable_layout.txt     size, slot offsets and slot types of the reference's struct acceleration_functions and the type
                            of its init function (tests/native/vtable_layout_dump.cc; tests/test_vtable.py)

    python tools/ref_source_golden.py

Where the sources are present, the tests also check that these files still say what the sources say."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402  (REF_ROOT)

GOLD = os.path.join(ROOT, "tests", "golden")
TABLES_JSON = os.path.join(GOLD, "ref_tables.json")
LAYOUT_TXT = os.path.join(GOLD, "ref_vtable_layout.txt")
LAYOUT_SRC = os.path.join(ROOT, "tests", "native", "vtable_layout_dump.cc")

# name -> (source file under libde265/, declaration, number of values)
TABLES = {
    "mat_dct": ("fallback-dct.cc", r"static int8_t mat_dct\[32\]\[32\]", 1024),
    "mat_8_357": ("fallback-dct.cc", r"static int8_t mat_8_357\[4\]\[4\]", 16),
    "table_8_23_beta": ("deblock.cc", r"static uint8_t table_8_23_beta\[52\]", 52),
    "table_8_23_tc": ("deblock.cc", r"static uint8_t table_8_23_tc\[54\]", 54),
    "intraPredAngle_table": ("intrapred.cc", r"const int intraPredAngle_table\[1\+34\]", 35),
    "invAngle_table": ("intrapred.cc", r"static const int invAngle_table\[25-10\]", 15),
    "levelScale": ("transform.cc", r"static const int levelScale\[\]", 6),
    "tab8_22": ("transform.cc", r"const int tab8_22\[\]", 14),
}


def have_sources():
    return pyref.can_build()


def _ref_array(fname, decl_regex, count):
    txt = open(os.path.join(pyref.REF_ROOT, "libde265", fname)).read()
    m = re.search(decl_regex + r"[^=]*=\s*\{(.*?)\};", txt, re.S)
    assert m, decl_regex
    body = re.sub(r"//.*", "", m.group(1))
    nums = [int(x) for x in re.findall(r"-?\d+", body)]
    assert len(nums) == count, (decl_regex, len(nums))
    return nums


def tables_from_sources():
    return {name: _ref_array(*spec) for name, spec in TABLES.items()}


def stored_tables():
    return json.load(open(TABLES_JSON))["tables"]


def vtable_layout(against_reference=False):
    """Output of tests/native/vtable_layout_dump.cc, built with g++ against the product's header or the reference's."""
    if against_reference:
        ref = pyref.REF_ROOT
        inc = ["-DAGAINST_REFERENCE", "-I%s/libde265" % ref, "-I%s" % ref, "-idirafter", "%s/extra" % ref]
    else:
        inc = ["-I%s/include" % ROOT]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "vtable_layout_dump")
        r = subprocess.run(["g++", "-std=c++11", "-w"] + inc + [LAYOUT_SRC, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout


def stored_vtable_layout():
    return open(LAYOUT_TXT).read()


def main():
    if not have_sources():
        raise SystemExit("the reference sources are not at %s (DE265_REFERENCE)" % pyref.REF_ROOT)
    with open(TABLES_JSON, "w") as f:
        json.dump({"_generated_by": "python tools/ref_source_golden.py", "tables": tables_from_sources()}, f)
        f.write("\n")
    with open(LAYOUT_TXT, "w") as f:
        f.write(vtable_layout(against_reference=True))
    print("wrote", TABLES_JSON, LAYOUT_TXT)


if __name__ == "__main__":
    main()
