"""gfx950 assembly listings of the library's sources and what the compiler says about every kernel in them: the one compile-and-parse
module behind the build-quality gates (tests/test_*kernel_resources.py) and behind isa_same.py / isa_report.py.  No GPU needed.

    listing(source, extra=())           the listing of csrc/<source>, compiled by stnerf_amd.build.device_asm (the build's own flags)
    listing_of(code, like)              the listing of source text (a gate's probe kernel), compiled with the flags of the source `like`
    kernels(text)                       {symbol: record} of a listing, in the listing's order
    assert_no_scratch_no_call(k, name)  what most gates ask of a kernel's instructions
    needs_hipcc                         the gates' pytest marker: skip where there is no compiler

A record is a dict: "body", the text from the kernel's label up to its (first) s_endpgm; the integer lines of the summary the compiler
prints behind the kernel (NumVgprs, NumAgprs, TotalNumVgprs, TotalNumSgprs, ScratchSize, Occupancy, LDSByteSize, ...); and the integer
fields of the kernel's own ``amdhsa.kernels`` record, found by its .name (vgpr_count, agpr_count, private_segment_fixed_size,
group_segment_fixed_size, vgpr_spill_count, sgpr_spill_count, ...).  Reading a field the listing does not hold is a KeyError."""
import atexit
import functools
import os
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from stnerf_amd import build  # noqa: E402

TIMEOUT = 900          # seconds per compile (mlp_bf16x3.hip takes 45 s on an idle build machine)


@functools.lru_cache(maxsize=None)
def _tmp():
    d = tempfile.mkdtemp(prefix="stnerf_asm_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _compiled(source, extra, code=None):
    d = tempfile.mkdtemp(dir=_tmp())
    path = None
    if code is not None:
        path = os.path.join(d, "probe.hip")
        with open(path, "w") as f:
            f.write(code)
    with open(build.device_asm(source, os.path.join(d, "listing.s"), extra=extra, path=path, quiet=True, timeout=TIMEOUT)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def listing(source, extra=()):
    """Compiled once per process and (source, extra); `extra` is a tuple of flags."""
    return _compiled(source, extra)


@functools.lru_cache(maxsize=None)
def listing_of(code, like):
    return _compiled(like, (), code)


def kernels(text):
    metadata = {}
    for rec in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        rec = "    " + rec          # a record's own fields sit four columns in (the first one behind the dash), its arguments' deeper
        named = re.search(r"^    \.name:\s+(\S+)", rec, re.M)
        if named:                   # (not: the entries of amdhsa.version behind the kernels)
            metadata[named.group(1)] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", rec, re.M)}
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        label = re.search(r"^" + re.escape(name) + r":", text, re.M)
        end = text.index("s_endpgm", label.start())
        nxt = text.find("; -- Begin function", end)              # the kernel's summary lies in front of the next function
        record = {"body": text[label.start():end]}
        for k, v in re.findall(r"^; (\w+): (\d+)\b", text[end:nxt if nxt >= 0 else len(text)], re.M):
            record.setdefault(k, int(v))
        record.update(metadata[name])
        out[name] = record
    return out


def assert_no_scratch_no_call(kernel, name):
    assert "scratch_" not in kernel["body"] and "s_swappc" not in kernel["body"], name


def __getattr__(name):
    if name == "needs_hipcc":          # (here, so that the tools import no pytest)
        import pytest
        return pytest.mark.skipif(shutil.which(build._hipcc()) is None, reason="no hipcc")
    raise AttributeError(name)
