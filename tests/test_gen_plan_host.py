"""CPU: the planner of the general-index engine (alchemy_amd/csrc/gen_host.hpp: gen_plan) in a stand-alone program
(tests/sanitize/gen_plan_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  For every index
2^a 3^b 5^c 7^d 11^e 13^f with m != 2 (mod 4) and phi(m) <= 65535 (1972 indices, 1645 of them within the 160 KiB that alch_ring_create
serves at 4-byte words): the plan succeeds within its array bounds, the group sizes of every axis multiply to its length, every stride
follows the documented rule, and fdiv -- the mulhi by floor(2^32 / d) + 1 every pass and every column recurrence divides with -- equals
`/` for every dividend a kernel can form, exhaustively, at the plan's own reciprocals.

The same program prints the plans of the indices of tests/test_gpu_general_structure.py, and the second test asserts that every one
of them has the structural property its row gives as its reason; the size selectors (gen_threads' two constants, the fused key
switch's bound, the LDS limit) are read from the sources by regular expression, so a retune makes this test name the rows to move."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "alchemy_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gen_plan") / "gen_plan_harness")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")             # the default of alchemy_amd/csrc/Makefile
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "sanitize", "gen_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    return out.stdout


def test_every_served_index_plans_within_bounds_and_divides_exactly(harness):
    out = run(harness).strip().split("\n")
    assert out[-1] == "OK: 0 failed expectation(s)", "\n".join(out[-25:])
    assert out[-2] == "planned 1972 indices, 1645 with phi <= 40960, 1249 with phi <= 20480"


# ---- the size selectors, from the sources --------------------------------------------------------------------------------------------
def selectors():
    gen = open(os.path.join(CSRC, "kernel_gen.hpp")).read()
    lib = open(os.path.join(CSRC, "alchemy_hip.hip")).read()

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    body = gen[gen.index("inline int gen_threads("):]
    body = body[:body.index("\n}\n")]
    wide = one(r"if \(bytes > (\d+)\) return 512;", body)
    small = one(r"#define ALCH_GEN_SMALL_BYTES (\d+)", body)
    assert "return bytes <= ALCH_GEN_SMALL_BYTES ? GEN_T_SMALL : GEN_T;" in body
    assert one(r"constexpr int GEN_T_SMALL = (\d+);", gen) == 128 and one(r"constexpr int GEN_T = (\d+);", gen) == 256
    ks = one(r"constexpr int GEN_KS_T = (\d+);", gen) * one(r"constexpr int GEN_KS_NPT = (\d+);", gen)
    assert "r->n <= (u32)(GEN_KS_T * GEN_KS_NPT)" in lib              # gen_ks_fused: the bound of the fused general key switch
    lds = one(r"\(size_t\)gh\.n \* \(size_t\)word > (\d+)\) return fail\(ALCH_E_UNSUPPORTED", lib)
    return {"small": small, "wide": wide, "ks": ks, "lds": lds}


def gen_threads(phi, word, sel):
    """gen_threads of kernel_gen.hpp with gen_nt = 0, restated."""
    b = phi * word
    return 512 if b > sel["wide"] else 128 if b <= sel["small"] else 256


def parse_plans(text):
    plans, cur = {}, None
    for ln in text.strip().split("\n"):
        t = ln.split()
        if t[0] == "index":
            assert t[2] == "n", ln                                       # "index M refused ..." would fail here
            cur = {"n": int(t[3]), "fact": [], "pass": []}
            plans[int(t[1])] = cur
        elif t[0] == "fact":
            cur["fact"].append({k: int(v) for k, v in zip(t[2::2], t[3::2])})
        elif t[0] == "pass":
            d = dict(zip(t[2::2], t[3::2]))
            cur["pass"].append({k: (v if k == "kind" else int(v)) for k, v in d.items()})
    return plans


def holds(prop, plan, word, sel):
    """One property word of tests/test_gpu_general_structure.py on one plan."""
    n, passes, facts = plan["n"], plan["pass"], plan["fact"]
    vl = 16 // word
    inner = [p for p in passes if p["stride"] == 1]
    assert len(inner) == 1                                               # exactly one pass walks the innermost axis at stride 1
    inner = inner[0]
    kinds = {"crt": "SYM_CRT", "dft": "SYM_DFT"}
    t = prop.split(":")
    if t[0] == "crt":
        return any(p["kind"] == "SYM_CRT" and p["r"] == int(t[1]) - 1 for p in passes)
    if t[0] == "dft":
        return sum(p["kind"] == "SYM_DFT" and p["r"] == int(t[1]) for p in passes) == int(t[2])
    if t[0] == "inner":
        return inner["kind"] == kinds[t[1]] and inner["r"] == int(t[2])
    if t[0] == "strided":
        return inner["r"] % vl != 0
    if t[0] == "contig":
        return inner["kind"] != "R2BLOCK" and inner["r"] == int(t[1]) and inner["r"] % vl == 0
    if t[0] == "outer":
        return facts[0]["p"] == int(t[1]) and len(facts) > 1
    if t[0] == "last":
        return facts[-1]["p"] == int(t[1]) and len(facts) > 1
    if t[0] == "tail":
        blocks = [p for p in passes if p["kind"] == "R2BLOCK"]
        return bool(blocks) and blocks[-1]["r"] == 1 << int(t[1]) and len(facts) > 1 and passes[len(blocks)]["kind"] == "SYM_CRT"
    if t[0] == "one_group":
        return all(p["groups"] == 1 for p in passes)
    if t[0] == "groups<128":
        return all(p["groups"] < 128 for p in passes)
    if t[0] == "scalar":
        return n % vl != 0
    if t[0] == "vector":
        return n % vl == 0
    if t[0] == "nt":
        return gen_threads(n, word, sel) == int(t[1])
    if t[0] == "fused":
        return n <= sel["ks"]
    if t[0] == "composed":
        return n > sel["ks"]
    if t[0] == "lds_full":
        return n * word == sel["lds"]
    if t[0] == "npass":
        return len(passes) == int(t[1])
    raise AssertionError(f"unknown property {prop}")


def test_every_index_of_the_structure_file_has_the_property_it_was_chosen_for(harness):
    import test_gpu_general_structure as TS
    sel = selectors()
    indices = sorted({m for r, _ in TS.ROWS.values() for m in r.indices} | {m for m, _, _ in TS.REFUSED})
    plans = parse_plans(run(harness, *[str(m) for m in indices]))
    wrong = []
    for name, (r, props) in TS.ROWS.items():
        assert set(props) == set(r.indices), name                       # every index of the row states its reason
        for m in r.indices:
            assert plans[m]["n"] * r.word <= sel["lds"], (name, m)
            wrong += [f"row {name}, index {m} (phi {plans[m]['n']}, {r.word}-byte words): not `{p}`" for p in props[m].split()
                      if not holds(p, plans[m], r.word, sel)]
    assert not wrong, "move these rows of tests/test_gpu_general_structure.py:\n" + "\n".join(wrong)
    # the rows sit NEXT to their thresholds: within 2 % of the selector, one index on either side
    p32 = {m: plans[m]["n"] * 4 for m in plans}
    p64 = {m: plans[m]["n"] * 8 for m in plans}
    assert p32[15876] <= sel["small"] < p32[13824] and p32[13824] - p32[15876] < sel["small"] // 50
    assert p32[42240] <= sel["wide"] < p32[31104] and p32[31104] - p32[42240] < sel["wide"] // 50
    assert p64[3969] <= sel["small"] < p64[5824] and p64[5824] - p64[3969] < sel["small"] // 50
    assert p64[21120] <= sel["wide"] < p64[12285] and p64[12285] - p64[21120] < sel["wide"] // 50
    assert plans[53760]["n"] == sel["ks"] < plans[21609]["n"] < plans[14641]["n"] < sel["ks"] * 11 // 10
    # the battery covers what the rows promise: every odd prime's CRT and DFT pass at either word size, every tail length, both loaders
    for word in (4, 8):
        rows = [(r, props) for r, props in TS.ROWS.values() if r.word == word]
        said = {p for r, props in rows for m in r.indices for p in props[m].split()}
        for p in (3, 5, 7, 11, 13):
            assert f"crt:{p}" in said or any(s.startswith(f"contig:{p - 1}") or s == f"inner:crt:{p - 1}" for s in said), (word, p)
            assert any(s.startswith(f"dft:{p}:") for s in said), (word, p)
    said4 = {p for r, props in TS.ROWS.values() if r.word == 4 for m in r.indices for p in props[m].split()}
    assert {"tail:1", "tail:2", "tail:3", "scalar", "vector", "one_group", "groups<128", "contig:4", "contig:12", "lds_full", "fused",
            "composed", "nt:128", "nt:256", "nt:512"} <= said4
    assert {f"inner:crt:{p - 1}" for p in (3, 7, 11)} <= said4 and {f"outer:{p}" for p in (2, 3, 5, 7, 11)} <= said4
    said8 = {p for r, props in TS.ROWS.values() if r.word == 8 for m in r.indices for p in props[m].split()}
    assert {"contig:2", "contig:6", "contig:10", "lds_full", "nt:128", "nt:256", "nt:512"} <= said8
    # refused: one step past the limit at the stated word size, inside gen_plan's own bound (so the size check is what refuses)
    for m, phi, word in TS.REFUSED:
        assert plans[m]["n"] == phi and phi * word > sel["lds"] and phi <= 65535
        assert word == 4 or phi * 4 <= sel["lds"]
