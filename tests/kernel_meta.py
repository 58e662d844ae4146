"""What the compiler says about the kernels of one source, for the tests that hold them to a budget: hipcc -S cross-compiles for
gfx950 without a GPU, and the assembly carries each kernel's register, spill, scratch and LDS figures as metadata.  Each
(source, extra flags) pair is compiled once per process; kernels are looked up by their exact name, read from the mangled symbol's
length prefix, so k_play cannot hit k_cap_play.  tests/test_kernel_resources.py holds the table of budgets."""
import collections
import os
import re
import subprocess
import tempfile

from betazero_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = build.hipcc()
# the product library's code generation, to assembly instead of to a shared object
FLAGS = [f for f in build.FLAGS if f != "-shared"] + ["--cuda-device-only", "-S"]

COMMANDS = []   # every hipcc command line run, in order
_CACHE = {}     # (src, extra) -> Asm
_TMP = tempfile.TemporaryDirectory(prefix="kernel_meta_")   # the assembly files go here; removed when the process ends

_FIELDS = {"vgpr": "vgpr_count", "vspill": "vgpr_spill_count", "sspill": "sgpr_spill_count", "scratch": "private_segment_fixed_size",
           "lds_static": "group_segment_fixed_size", "max_wg": "max_flat_workgroup_size"}


class Asm:
    """.asm: the assembly text; .kernels: mangled symbol -> {vgpr, agpr, vspill, sspill, scratch, lds_static, max_wg}"""

    def __init__(self, asm):
        self.asm = asm
        self.kernels = {}
        for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                k = {f: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1)) for f, key in _FIELDS.items()}
                k["agpr"] = int(re.match(r"\s*(\d+)", blk).group(1))
                self.kernels[name.group(1)] = k

    def body(self, symbol):
        """the text from the kernel's label to its s_endpgm"""
        m = re.search(rf"^{re.escape(symbol)}:\s*; @{re.escape(symbol)}$", self.asm, re.M)
        assert m, symbol
        return self.asm[m.end():self.asm.index("s_endpgm", m.end())]

    def find(self, name, *template_parts):
        return find(self.kernels, name, *template_parts)

    def count(self, symbol, mnemonic):
        """occurrences of an instruction in one kernel's body"""
        return len(re.findall(rf"^\s+{mnemonic}\b", self.body(symbol), re.M))


def compile_asm(src, extra=()):
    key = (src, tuple(extra))
    if key not in _CACHE:
        out = os.path.join(_TMP.name, f"{len(COMMANDS)}_{src}.s")
        cmd = [HIPCC, *FLAGS, *extra, "-o", out, os.path.join(ROOT, "betazero_amd", "csrc", src)]
        COMMANDS.append(cmd)
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        with open(out) as f:
            _CACHE[key] = Asm(f.read())
    return _CACHE[key]


def split_symbol(symbol):
    """(base name, template-argument part) of a mangled function symbol: _Z, an optional N, then length-prefixed names, the last
    of which is the function's; its template arguments, if any, are the balanced I...E that follows (returned with the I and E)"""
    m = re.match(r"_ZN?", symbol)
    if not m:
        return symbol, ""
    i, name = m.end(), None
    while (d := re.match(r"\d+", symbol[i:])):
        n = int(d.group())
        name = symbol[i + d.end():i + d.end() + n]
        i += d.end() + n
    if name is None:
        return symbol, ""
    if symbol[i:i + 1] != "I":
        return name, ""
    start, depth = i, 0
    while i < len(symbol):
        lit = re.match(r"L[a-z]n?\d+E", symbol[i:])      # a literal of a builtin type, Li128E or Lb1E: its digits are no length
        d = re.match(r"\d+", symbol[i:])
        if lit:
            i += lit.end()
        elif d:
            i += d.end() + int(d.group())
        else:
            depth += {"I": 1, "N": 1, "E": -1}.get(symbol[i], 0)
            i += 1
            if depth == 0:
                return name, symbol[start:i]
    raise AssertionError(f"unbalanced template arguments in {symbol}")


def matches(kernels, name, *template_parts):
    """the symbols whose function is called exactly `name` and whose template arguments contain every part"""
    hits = []
    for sym in kernels:
        base, targs = split_symbol(sym)
        if base == name and all(p in targs for p in template_parts):
            hits.append(sym)
    return hits


def find(kernels, name, *template_parts):
    hits = matches(kernels, name, *template_parts)
    assert len(hits) == 1, (name, template_parts, hits)
    return hits[0]


class Row(collections.namedtuple("Row", "name parts vgpr agpr zero")):
    """one kernel instantiation's budget: vgpr / agpr are None, ("==", n) or ("<=", n); the fields in `zero` must be 0"""

    def __str__(self):
        return "-".join((self.name,) + self.parts)


def row(name, *parts, vgpr=None, agpr=None, zero=()):
    return Row(name, parts, vgpr, agpr, tuple(zero))


def check(kernels, r):
    """what of row r does not hold in `kernels`: a list of messages, empty when all is well"""
    hits = matches(kernels, r.name, *r.parts)
    if len(hits) != 1:
        return [f"{r}: {len(hits)} kernels match, want exactly one: {hits}"]
    k, bad = kernels[hits[0]], []
    for field in ("vgpr", "agpr"):
        want = getattr(r, field)
        if want is not None:
            op, n = want
            assert op in ("==", "<=")
            if not (k[field] == n if op == "==" else k[field] <= n):
                bad.append(f"{r}: {field} is {k[field]}, want {op} {n}")
    for field in r.zero:
        if k[field] != 0:
            bad.append(f"{r}: {field} is {k[field]}, want 0")
    return bad
