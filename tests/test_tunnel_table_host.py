"""CPU: the index tables of a general-index tunnel (alchemy_amd/csrc/gen_host.hpp: gen_tunnel_table) in a stand-alone program
(tests/sanitize/tunnel_table_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  For every ordered pair r' != s'
of indices 2^a 3^b 5^c 7^d 11^e 13^f with both phi <= 384: d_rel phi(e') = phi(r'), the rows of `table` hit every position of R' exactly
once, table_e is `table` without its gaps, slot_e is a phi(s') / phi(e') to one map onto the slots of E', and linv_skip_mask names the
primes of r' that divide e'.  (The issue asked for phi <= 2048; one pair's table has d_rel phi(s') entries, the walk grows with the
fourth power of the bound and takes a minute there under the sanitizers: 384 keeps it to a few seconds and still has 7^3, 11^2, 13^2
and five-prime indices on either side.)

The same program prints, for the pairs of tests/test_gpu_tunnel_structure.py, what alch_tunnel_create and do_tunnel decide from the
pair alone; the second test asserts that every pair has the property its row gives as its reason.  The thresholds (GEN_TUN_T, the
NP dispatch, the 65536-byte bounds of `fused` and `tun_ng`) are read from the sources by regular expression, so a retune makes this
test name the rows to move."""
import math
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "alchemy_amd", "csrc")
PHI_MAX = 384


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tunnel_table") / "tunnel_table_harness")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")             # the default of alchemy_amd/csrc/Makefile
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", f"-DPHI_MAX={PHI_MAX}", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "sanitize", "tunnel_table_harness.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    return out.stdout


def test_every_pair_of_small_indices_builds_consistent_tables(harness):
    out = run(harness).strip().split("\n")
    assert out[-1] == "OK: 0 failed expectation(s)", "\n".join(out[-25:])
    found = re.fullmatch(r"walked (\d+) pairs of (\d+) indices with phi <= (\d+): (\d+) with e' = 1, (\d+) with e' = s', (\d+) with e' = r'", out[-2])
    assert found, out[-2]
    pairs, indices, bound, e1, es, er = map(int, found.groups())
    assert bound == PHI_MAX and pairs == indices * (indices - 1) and indices > 150 and e1 > 5000 and es == er > 1000


# ---- the thresholds, from the sources -------------------------------------------------------------------------------------------------
def selectors():
    gen = open(os.path.join(CSRC, "kernel_gen.hpp")).read()
    lib = open(os.path.join(CSRC, "alchemy_hip.hip")).read()

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]

    T = int(one(r"constexpr int GEN_TUN_T = (\d+);", gen))
    nps = [int(x) for x in re.findall(r"if \(pieces <= (\d+)\) return ng == 4 \? gen_launch_tunnel_ks_t<W, 4, (?:\d+)>", gen)]
    assert len(nps) == 2 and nps[0] < nps[1]
    assert all(f"gen_launch_tunnel_ks_t<W, 4, {n}>(R, GE, A, nct, stream) : gen_launch_tunnel_ks_t<W, 2, {n}>" in gen for n in nps)
    last, lds = one(r"rs->n <= \(u32\)\(GEN_TUN_T \* 4 \* (\d+)\) && 2 \* \(size_t\)rx->n \* sizeof\(W\) <= (\d+);", lib)
    assert f"gen_launch_tunnel_ks_t<W, 4, {last}>(R, GE, A, nct, stream) : gen_launch_tunnel_ks_t<W, 2, {last}>" in gen and int(last) > nps[1]
    ng_lds = int(one(r"rs->opts\.tunnel_fused == 4 && 4 \* \(size_t\)rx->n \* sizeof\(W\) <= (\d+)\) \? 4 : 2;", lib))
    return {"T": T, "np": nps + [int(last)], "lds": int(lds), "ng_lds": ng_lds}


def fused_class(rec, sel):
    """`fused`, `tun_ng` of do_tunnel and the dispatch of gen_launch_tunnel_ks at 4-byte words, restated."""
    phis, phie = rec["phi_s"], rec["phi_e"]
    if not (rec["e_ring"] and rec["pieces_ok"] and phis % 4 == 0 and phie % 4 == 0 and phis <= sel["T"] * 4 * sel["np"][-1] and 2 * phie * 4 <= sel["lds"]):
        return "none"
    pieces = (phis // 4 + sel["T"] - 1) // sel["T"]
    return f"{4 if 4 * phie * 4 <= sel['ng_lds'] else 2}/{next(n for n in sel['np'] if pieces <= n)}"


def parse(text):
    out = {}
    for ln in text.strip().split("\n"):
        t = ln.split()
        assert t[0] == "pair" and t[3] != "refused", ln
        rec = {k: int(v) for k, v in zip(t[3:-2:2], t[4:-2:2])}
        assert t[-2] == "fused"
        rec["fused"] = t[-1]
        out[(int(t[1]), int(t[2]))] = rec
    return out


def holds(prop, pair, rec):
    rp, sp = pair
    t = prop.split(":")
    if t[0] == "e":
        return rec["ep"] == int(t[1])
    if prop == "e=s":
        return rec["ep"] == sp
    if prop == "e=r":
        return rec["ep"] == rp and rec["d_rel"] == 1
    if t[0] == "drel":
        return rec["d_rel"] == int(t[1])
    if t[0] in ("phis", "phie", "phir"):
        return rec["phi_" + t[0][-1]] == int(t[1])
    if t[0] in ("phis%4", "phie%4"):
        return rec["phi_" + t[0][3]] % 4 == int(t[1])
    if prop in ("ering", "noering"):
        return rec["e_ring"] == (prop == "ering")
    if prop == "e2pow":
        return rec["ep"] >= 32 and rec["ep"] & (rec["ep"] - 1) == 0 and rp & (rp - 1) and sp & (sp - 1)
    if t[0] == "pieces":
        return rec["pieces_ok"] == int(t[1])
    if t[0] == "dec":
        return rec["dec_c0"] == int(t[1])
    if t[0] == "fused":
        return rec["fused"] == t[1]
    if prop == "nofused":
        return rec["fused"] == "none"
    if prop == "p11":
        return (rp * sp) % 11 == 0
    raise AssertionError(f"unknown property {prop}")


def test_every_pair_of_the_structure_file_has_the_property_it_was_chosen_for(harness):
    import test_gpu_tunnel_structure as TS
    sel = selectors()
    rows = {**TS.ROWS, **TS.LARGE_ROWS}
    pairs = [p for row in rows.values() for p in row]
    assert len(set(pairs)) == len(pairs)
    recs = parse(run(harness, *[f"{r}:{s}" for r, s in pairs + [(40, 60), (63, 105)]]))
    wrong = []
    for name, row in rows.items():
        for pair, props in row.items():
            rec = recs[pair]
            assert rec["ep"] == math.gcd(*pair) and rec["d_rel"] * rec["phi_e"] == rec["phi_r"]
            assert rec["fused"] == fused_class(rec, sel), (pair, rec, fused_class(rec, sel))       # the program's constants are the sources'
            wrong += [f"row {name}, pair {pair[0]} -> {pair[1]}: not `{p}` ({rec})" for p in props.split() if not holds(p, pair, rec)]
    assert not wrong, "move these rows of tests/test_gpu_tunnel_structure.py:\n" + "\n".join(wrong)
    # the size rows sit ON their thresholds and just past them (within 2 %)
    phis = {p: recs[p]["phi_s"] for p in pairs}
    phie = {p: recs[p]["phi_e"] for p in pairs}
    T4 = sel["T"] * 4
    n3, n5, n6 = sel["np"]
    assert phis[(35, 23040)] == T4 * n3 < phis[(1183, 9295)] < T4 * n3 * 51 // 50
    assert phis[(175, 25600)] == phis[(38400, 25600)] == T4 * n5 < phis[(35, 38880)] < T4 * n5 * 51 // 50
    assert phis[(35, 46080)] == phis[(39936, 26624)] == T4 * n6 < phis[(676, 27885)] < T4 * n6 * 51 // 50
    assert 16 * phie[(30720, 20480)] == sel["ng_lds"] < 16 * phie[(36015, 28812)] < sel["ng_lds"] * 51 // 50
    # 2 phi(e') 4 <= lds can never bind: e' is a proper divisor of s' with both dimensions even multiples, so phi(e') <= phi(s') / 2
    assert 2 * (T4 * n6 // 2) * 4 <= sel["lds"]
    # all six instantiations, every form's fall-back reason, both values of dec_c0 with and without an E' ring, the prime 11 in every form
    said = {(recs[p]["fused"], recs[p]["e_ring"], recs[p]["pieces_ok"], recs[p]["dec_c0"]) for p in pairs}
    # (NG = 2 with NP = 3 needs phi(e') > 4096 under phi(s') <= 6144 and does not exist under tunnel_fused = 4; the option set
    # tunnel_fused = 2 of the battery runs NG = 2 on every fused pair, the NP = 3 ones among them)
    assert {f"{g}/{n}" for g in (2, 4) for n in sel["np"]} - {f"2/{n3}"} == {s[0] for s in said} - {"none"}
    assert 4 * (T4 * n3 // 2) * 4 <= sel["ng_lds"]
    assert {(e, pc, d) for _, e, pc, d in said} == {(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)}
    with11 = {(recs[p]["e_ring"], recs[p]["pieces_ok"]) for p in pairs if (p[0] * p[1]) % 11 == 0}
    assert with11 == {(0, 0), (1, 0), (1, 1)}
    assert {recs[p]["d_rel"] for p in pairs} >= {1, 2, 3, 4, 5, 6, 7, 11}
    # the pairs the suite pinned before this file: the shapes the issue says they have
    assert (recs[(40, 60)]["fused"], recs[(63, 105)]["pieces_ok"], recs[(63, 105)]["e_ring"]) == ("4/3", 0, 1)
    # refused pairs: a two-power index >= 32 on one side only
    for rp, sp in TS.REFUSED:
        assert (rp >= 32 and rp & (rp - 1) == 0) != (sp >= 32 and sp & (sp - 1) == 0)
    # the battery's lists name pairs of the table
    assert set(TS.DUP_PAIRS) <= set(pairs) and set(TS.SMALL) | set(TS.LARGE) == set(pairs)
    assert all(recs[p]["phi_s"] <= 120 for p in TS.SMALL) and all(recs[p]["phi_s"] >= 6144 for p in TS.LARGE)
