"""sqlite_abi.py — the numbers sqlite-muninn_amd/ext/mn_sqlite_abi.h hard-codes: sqlite3_api_routines slot numbers and the
sizes / offsets of the vtab structs, printed by a small C program compiled against a header.  gen_golden.py records them from a
genuine sqlite3ext.h (tests/golden/sqlite_abi.json); tests/test_sqlite_ext.py compiles the hand-written header and compares.
TEST INFRASTRUCTURE ONLY."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_H = os.path.join(ROOT, "sqlite-muninn_amd", "ext", "mn_sqlite_abi.h")
LAYOUT = ("sizeof(sqlite3_module)", "sizeof(sqlite3_vtab)", "sizeof(sqlite3_vtab_cursor)", "sizeof(sqlite3_index_info)",
          "sizeof(struct sqlite3_index_constraint)", "sizeof(struct sqlite3_index_orderby)",
          "sizeof(struct sqlite3_index_constraint_usage)", "offsetof(sqlite3_index_info, aConstraintUsage)",
          "offsetof(sqlite3_index_info, idxNum)", "offsetof(sqlite3_index_info, estimatedCost)",
          "offsetof(sqlite3_index_info, estimatedRows)", "offsetof(sqlite3_module, xUpdate)",
          "offsetof(sqlite3_module, xFilter)", "offsetof(sqlite3_vtab, zErrMsg)")


def declared_slots():
    """{routine: slot number} as mn_sqlite_abi.h declares them (MN_SLOT_<routine>)"""
    return {k: int(v) for k, v in re.findall(r"#define MN_SLOT_(\w+) (\d+)", open(ABI_H).read())}


def measure(header, workdir, slots=()):
    """compile a program that includes `header` and return ({routine: slot number} for `slots`, [layout values])"""
    body = "\n".join(f'printf("S {k} %zu\\n", offsetof(struct sqlite3_api_routines, {k}) / sizeof(void *));' for k in slots)
    lay = "\n".join(f'printf("L %zu\\n", (size_t)({e}));' for e in LAYOUT)
    src = os.path.join(workdir, "abi.c")
    exe = os.path.join(workdir, "abi")
    with open(src, "w") as f:
        f.write(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{\n{body}\n{lay}\nreturn 0;}}\n')
    subprocess.run(["gcc", "-o", exe, src], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[1]: int(l.split()[2]) for l in lines if l.startswith("S ")}
    return got, [int(l.split()[1]) for l in lines if l.startswith("L ")]
