"""CPU suite: the Python binding's hand-written mirror of include/qldpc.h against the header itself -- the layout of every struct (a C program
compiled with the host compiler prints sizes and offsets), the argument count of every prototype, and the names the package has always had.
No GPU, no device."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qldpc.h")

# header struct -> the attribute of the package that mirrors it (a ctypes.Structure or a numpy dtype)
MIRRORS = {
    "qldpc_decoder_cfg": "DecoderCfg", "qldpc_kernel_stat": "KernelStat", "qldpc_qber_cfg": "QberCfg",
    "qldpc_recon_cfg": "ReconCfg", "qldpc_recon_msg": "ReconMsg", "qldpc_recon_blind": "ReconBlind", "qldpc_recon_guess": "RECON_GUESS_DTYPE",
    "qldpc_toeplitz_cfg": "_ToeplitzCfg", "qldpc_polyhash_cfg": "_PolyHashCfg",
    "qldpc_mc_cfg": "McCfg", "qldpc_mc_result": "McResult", "qldpc_mc_channel": "McChannel",
    "qldpc_mc_search_cfg": "McSearchCfg", "qldpc_mc_search_result": "McSearchResult", "qldpc_mc_pattern_stat": "MC_PATTERN_STAT",
    "qldpc_mc_point": "McPoint", "qldpc_mc_sweep_cfg": "McSweepCfg", "qldpc_mc_sweep_result": "McSweepResult", "qldpc_mc_point_stat": "MC_POINT_STAT",
    "qldpc_mc_table_point": "McTablePoint", "qldpc_mc_sweep_tables_cfg": "McSweepTablesCfg",
    "qldpc_mc_strata_cfg": "McStrataCfg", "qldpc_mc_stratum_stat": "MC_STRATUM_STAT",
    "qldpc_mc_blind_cfg": "McBlindCfg", "qldpc_mc_blind_result": "McBlindResult", "qldpc_mc_blind_round_stat": "MC_BLIND_ROUND_STAT",
    "qldpc_mc_guess_cfg": "McGuessCfg", "qldpc_mc_guess_result": "McGuessResult",
}
NOT_MIRRORED = set()                                    # structs of the header the binding has no use for: none today
UNBOUND = {"qldpc_qber_repeat_table_host"}              # prototypes of the header the binding does not call


def header_text():
    text = open(HEADER).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def header_structs():
    """{typedef name: [field names in order]} of the header's `typedef struct [tag] { ... } NAME;` blocks"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", header_text()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            fields += [re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", part).group(1) for part in decl.split(",")]
        out[name] = fields
    return out


def header_prototypes():
    """{function name: number of parameters} of the header's qldpc_*(...) prototypes"""
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", header_text())
    out = {}
    for name, params in re.findall(r"\b(qldpc_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, "%s is declared twice" % name
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{struct: (size, [(field, offset, size)])} as the host compiler lays the header's structs out"""
    structs = header_structs()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "qldpc.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('    printf("S %s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f) for f in fields]
    lines += ["    return 0;", "}"]
    d = tmp_path_factory.mktemp("abi")
    src, exe = str(d / "layout.c"), str(d / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), "-o", exe, src], check=True)
    out = {}
    for row in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = row.split()
        if w and w[0] == "S":
            out[w[1]] = (int(w[2]), [])
        elif w:
            out[w[1]][1].append((w[2], int(w[3]), int(w[4])))
    return out


def mirror_layout(m):
    """(size, [(field, offset, size)]) of a ctypes.Structure or of a numpy dtype"""
    if isinstance(m, np.dtype):
        return m.itemsize, [(f, m.fields[f][1], m.fields[f][0].itemsize) for f in m.names]
    return C.sizeof(m), [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_]


def test_no_struct_of_the_header_is_forgotten():
    structs = set(header_structs())
    assert len(MIRRORS) >= 25 and not NOT_MIRRORED & set(MIRRORS)
    assert structs == set(MIRRORS) | NOT_MIRRORED, "structs of qldpc.h neither mirrored nor listed: %s; listed but gone: %s" % (
        sorted(structs - set(MIRRORS) - NOT_MIRRORED), sorted((set(MIRRORS) | NOT_MIRRORED) - structs))


@pytest.mark.parametrize("name", sorted(MIRRORS))
def test_struct_layout_is_the_headers(q, c_layout, name):
    size, fields = c_layout[name]
    assert len(fields) >= 1
    got_size, got_fields = mirror_layout(getattr(q, MIRRORS[name]))
    assert got_fields == fields, "%s / %s: (field, offset, size) differ" % (name, MIRRORS[name])
    assert got_size == size


@pytest.fixture(scope="module")
def bound():
    """{function: len(argtypes)} of what the binding itself gives a signature, from a fresh interpreter (tests bind functions of their own)"""
    code = ("import json, _qldpc_loader as l; q = l.load(); "
            "print(json.dumps({k: len(v.argtypes) for k, v in vars(q._L).items() if isinstance(v, q._L._FuncPtr) and v.argtypes is not None}))")
    return json.loads(subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, capture_output=True, text=True).stdout)


def test_every_prototype_is_bound_with_its_argument_count(bound):
    protos = header_prototypes()
    assert len(protos) >= 196
    assert {n for n in protos if n not in bound} == UNBOUND
    wrong = {n: (bound[n], protos[n]) for n in protos if n in bound and bound[n] != protos[n]}
    assert not wrong, "len(argtypes) against the prototype's parameters: %s" % wrong


def test_every_bound_name_is_in_the_header(bound):
    assert len(bound) >= 195
    assert not set(bound) - set(header_prototypes())


def test_the_package_keeps_its_names(q, gold):
    names = open(os.path.join(gold, "binding_names.txt")).read().split()
    assert len(names) >= 155
    assert not [n for n in names if not hasattr(q, n)]
