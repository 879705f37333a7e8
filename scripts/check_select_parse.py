"""The selector parser's host code under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone CPU program:
csrc/mn_select.hip and scripts/select_parse_main.cpp compiled with -Xarch_host -fsanitize=address,undefined, fed the recorded
grid of tests/test_select_model.py, that grid's texts cut short at every length, and 2 000 random strings; every answer is
compared with tests/select_model.py.  No device is touched.

    python scripts/check_select_parse.py
"""
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import select_model as sm  # noqa: E402
import test_select_model as tm  # noqa: E402


def model_line(text):
    try:
        prog = sm.parse(text)
    except sm.SelectError as e:
        return "E" + e.args[0].hex()
    out = "P"
    for op, name, up, down in prog:
        out += " %d:%d:%d:%s" % (op, up, down, (name or b"").hex())
    return out


def main():
    texts = [e.encode() for exprs in tm.selectors().values() for e in exprs]
    texts += [t[:k] for t in list(texts) if len(t) < 40 for k in range(len(t))]
    rng = random.Random(5)
    alphabet = [b"a", b"b", b"c", b"1", b"2", b"+", b"@", b",", b"not", b" ", b"\xff", b"9999999999"]
    texts += [b"".join(rng.choice(alphabet) for _ in range(rng.randint(1, 14))) for _ in range(2000)]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "select_parse")
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-Wno-unused-function", "-Wno-unused-value",
                        os.path.join(ROOT, "sqlite-muninn_amd", "csrc", "mn_select.hip"),
                        os.path.join(ROOT, "scripts", "select_parse_main.cpp"), "-o", exe], check=True)
        got = subprocess.run([exe], input="".join(t.hex() + "\n" for t in texts).encode(), stdout=subprocess.PIPE, check=True)
    lines = got.stdout.decode().splitlines()
    assert len(lines) == len(texts), (len(lines), len(texts))
    for t, line in zip(texts, lines):
        assert line == model_line(t), (t, line, model_line(t))
    print(len(texts), "selectors parsed under address,undefined sanitizers; every program and message equals the model's")


if __name__ == "__main__":
    main()
