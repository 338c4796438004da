"""The split-f16 format, the activation and the board I/O helpers are defined ONCE in csrc (tron_f16x3.hpp, tron_mish.hpp,
tron_codes_io.hpp): a kernel that needs one includes the header instead of copying it.  Checked on the source text alone:
for every helper name, exactly one definition (a regular expression on its signature) across csrc/*.hip and csrc/*.hpp,
and it sits in the header that owns it."""
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "deep-q-learning_tron_amd" / "csrc"

FUNCTIONS = {
    "tron_f16x3.hpp": ["split", "pack2", "wave_absmax", "absmax_scale", "lds_tr", "lds_tr_wait", "join8"],
    "tron_mish.hpp": ["mish_exact", "mish_grad_exact", "mish_fast", "mish4_capped", "mish_grad4_capped", "mish_grad_capped"],
    "tron_codes_io.hpp": ["chunk16", "load16", "store16"],
    "tron_conv_ws_kernel.hpp": ["stack_e"],
}
TYPEDEFS = {"tron_f16x3.hpp": ["f32x4", "u32x4", "s16x4", "f16", "f16x2", "f16x4", "f16x8"]}
CONSTANTS = {"tron_f16x3.hpp": ["ACT_SCALE", "ACT_UNSCALE", "LO_SCALE", "LO_UNSCALE"]}
# names the headers replaced: a definition under one of them is a copy coming back
GONE = ["mish1", "mish_grad1", "mish4", "mish_grad4", "lds_wait", "kstack_e", "grad_scale"]


def _sources():
    return sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.hpp")))


def _definitions(pattern):
    rx = re.compile(pattern, re.M)
    return [(p.name, m.group(0).strip()) for p in _sources() for m in rx.finditer(p.read_text())]


def _function(name):
    # "__device__ [__forceinline__] <return type> name(": a definition's or a declaration's signature, never a call
    return r"^[ \t]*(?:template[ \t]*<[^>\n]*>[ \t]*)?(?:static[ \t]+)?__device__[ \t]+(?:__forceinline__[ \t]+)?[\w:]+[ \t*&]+" + re.escape(name) + r"[ \t]*\("


CASES = (
    [(h, n, _function(n)) for h, names in FUNCTIONS.items() for n in names]
    + [(h, n, r"^[ \t]*typedef\b[^;\n]*[ \t*]" + re.escape(n) + r"\b(?:[ \t]+__attribute__\(\([^;\n]*\)\))?[ \t]*;")
       for h, names in TYPEDEFS.items() for n in names]
    + [(h, n, r"^[ \t]*constexpr[ \t]+float\b[^;\n]*\b" + re.escape(n) + r"[ \t]*=") for h, names in CONSTANTS.items() for n in names]
)


@pytest.mark.parametrize("header,name,pattern", CASES, ids=[c[1] for c in CASES])
def test_defined_once_in_its_header(header, name, pattern):
    assert _definitions(pattern) and [f for f, _ in _definitions(pattern)] == [header], (name, _definitions(pattern))


@pytest.mark.parametrize("name", GONE)
def test_replaced_name_not_defined(name):
    assert _definitions(_function(name)) == []


def test_no_second_name_for_the_wgrad_scale_or_f16x8():
    text = "".join(p.read_text() for p in _sources())
    assert not re.search(r"\bIN_SCALE\b|\bf16x8h\b", text)
