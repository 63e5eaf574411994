"""CPU-only: the parser of SITATOR_DEBUG_FILL (sitator_amd/csrc/debug_fill.h) compiled with the host compiler into a
stand-alone program under ASan / UBSan.  The knob is exactly two hexadecimal digits; everything else - a prefix, one or three
digits, the empty string, no variable at all - means off (-1), and the library then takes the path it always took."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv[1..]: texts to parse, one answer per line; no arguments: what debug_fill_byte() reads from the environment
PROBE = r"""
#include <stdio.h>
#include "debug_fill.h"

int main(int argc, char **argv)
{
    if (argc == 1) { printf("%d\n", debug_fill_byte()); return 0; }
    for (int i = 1; i < argc; i++) printf("%d\n", debug_fill_parse(argv[i]));
    printf("%d\n", debug_fill_parse(NULL));
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("debug_fill")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])
    return exe


CASES = [("ff", 0xFF), ("7B", 0x7B), ("0x7b", -1), ("", -1), ("zz", -1), ("100", -1),
         ("7b", 0x7B), ("00", 0), ("f", -1), ("7g", -1), (" 7b", -1), ("-1", -1), ("+f", -1)]


def test_two_hex_digits_and_nothing_else(probe):
    out = subprocess.run([probe] + [text for text, _ in CASES], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [want for _, want in CASES] + [-1]          # (the last line: a null pointer)


@pytest.mark.parametrize("value, want", [(None, -1), ("", -1), ("ff", 255), ("7B", 123), ("0x7b", -1), ("zz", -1), ("100", -1)])
def test_the_knob_is_read_from_the_environment_at_each_use(probe, value, want):
    env = {k: v for k, v in os.environ.items() if k != "SITATOR_DEBUG_FILL"}
    if value is not None:
        env["SITATOR_DEBUG_FILL"] = value
    out = subprocess.run([probe], check=True, capture_output=True, text=True, env=env).stdout
    assert int(out) == want
