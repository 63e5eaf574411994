"""CPU-only: k_fill3's launch planner (sitator_amd/csrc/fill3_plan.h) compiled with the host compiler, the way
test_abi.py compiles its probe of the public header.  What a plan must be comes from the build BEFORE the planner
existed: profiles/r08_plan_shapes_parent.txt is what that build launched on the MI355X (SITATOR_DEBUG_SHAPE=1 and sit_info
after every fill, SITATOR_FILL_AUTOTUNE=0; scratch/plan_shapes.py), profiles/r08_plan_shapes_parent_tune.txt the pairs its
autotune tried."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "r08_plan_shapes_parent.txt")
RECORD_TUNE = os.path.join(ROOT, "profiles", "r08_plan_shapes_parent_tune.txt")
LDS_LIMIT = 160 * 1024 - 256

# One case per input line: "name=value ..." for F3PlanIn, then "|", then "KNOB=value ..." (the environment, without
# the SITATOR_ prefix).  One output line per case: the line SITATOR_DEBUG_SHAPE prints, the rest of the plan, the pairs
# the autotune would try.
PROBE = r"""
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <iostream>
#include <sstream>
#include "fill3_plan.h"
int main()
{
    std::string line;
    std::vector<std::string> set;
    while (std::getline(std::cin, line)) {
        for (const std::string &k : set) unsetenv(k.c_str());
        set.clear();
        F3PlanIn in;
        memset(&in, 0, sizeof(in));
        std::istringstream ss(line);
        std::string tok;
        bool knobs = false;
        while (ss >> tok) {
            if (tok == "|") { knobs = true; continue; }
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (knobs) { setenv(("SITATOR_" + k).c_str(), v.c_str(), 1); set.push_back("SITATOR_" + k); continue; }
            const double d = strtod(v.c_str(), nullptr);
            const long long n = atoll(v.c_str());
            if (k == "S") in.S = n; else if (k == "M") in.M = n; else if (k == "vp") in.vp = (int)n; else if (k == "W") in.W = n;
            else if (k == "W_tight") in.W_tight = n; else if (k == "have_tight") in.have_tight = n != 0;
            else if (k == "mean") in.mean_candidates = d; else if (k == "tight_mean") in.tight_mean_candidates = d;
            else if (k == "dynmap") in.dynmap = n != 0; else if (k == "fuse_asked") in.fuse_asked = n != 0;
            else if (k == "fuse_ok") in.fuse_ok = n != 0; else if (k == "store") in.store = n != 0;
            else if (k == "f_lo") in.f_lo = n; else if (k == "f_hi") in.f_hi = n; else if (k == "F") in.F = n;
            else if (k == "idx_contig") in.idx_contig = n != 0; else if (k == "idx_s0") in.idx_s0 = n; else if (k == "idx_m0") in.idx_m0 = n;
            else if (k == "A") in.A = n; else if (k == "aligned") in.frames_aligned16 = n != 0; else if (k == "diag") in.diag = n != 0;
            else if (k == "ref_in_cell") in.f3_ref_in_cell = n != 0; else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const F3Knobs kn = f3_knobs_from_env();
        const F3Plan p = f3_plan(in, kn);
        if (p.err) { printf("error: %s\n", p.err); continue; }
        printf("k_fill3 shape: nw %d fpb %d rcap %d iw %d tt %d mcap %d, %zu bytes of LDS per workgroup", p.nw, p.fpb, p.rcap, p.iw, p.tt, p.mcap, p.lds);
        printf("; fuse %d slot_width %d slot %d contig %d store %d skipw %d prio %d rcap_auto %d tt_auto %d fpb1 %d total %d stop %d; cands", p.fuse, p.slot_width,
               p.slot, p.contig, p.store, p.skipw, p.prio, p.rcap_auto, p.tt_auto, p.fpb1, p.lay.total, f3_debug_stop(kn, in.dynmap));
        for (const std::pair<int, int> &q : f3_tune_candidates(p, in)) {
            const F3Plan t = f3_plan_with(p, q.first, q.second);
            printf(" %d:%d:%zu", t.rcap, t.tt, t.lds);
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("fill3_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(cases):
        """cases: [(dict of F3PlanIn fields, dict of knobs)] -> [dict of the plan]"""
        text = "".join("%s | %s\n" % (" ".join("%s=%s" % kv for kv in f.items()), " ".join("%s=%s" % kv for kv in k.items())) for f, k in cases)
        env = {k: v for k, v in os.environ.items() if not k.startswith("SITATOR_")}
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, env=env, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [parse(line) for line in out]
    return run


def parse(line):
    if line.startswith("error: "):
        return {"err": line[7:]}
    shape, rest, cands = line.split("; ")
    d = {"err": None, "shape": shape}
    d.update((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", shape.split(":", 1)[1].replace(" bytes", " 0").replace(",", "")))
    d["lds"] = int(re.search(r"(\d+) bytes", shape).group(1))
    d.update((k, int(v)) for k, v in re.findall(r"(\w+) (-?\d+)", rest))
    d["cands"] = [tuple(int(x) for x in c.split(":")) for c in cands.split()[1:]]
    return d


# ---- the parent's record ------------------------------------------------------------------------------------------------

def pad_vertices(vmax):
    vp = 4
    while vp < vmax:
        vp *= 2
    return vp


SHAPE = ("nw", "fpb", "rcap", "iw", "tt", "mcap", "lds", "fuse", "slot_width")


def read_facts(path):
    facts = {}
    for t in (line.split() for line in open(path) if line.startswith("facts ")):
        f = dict(zip(t[2::2], t[3::2]))
        facts[t[1]] = {"S": int(f["S"]), "M": int(f["M"]), "vp": pad_vertices(int(f["vmax"])), "W": int(f["W"]), "W_tight": int(f["W_tight"]),
                       "have_tight": int(float(f["delta"]) >= 0), "mean": f["mean_loose"], "tight_mean": f["mean_tight"]}
    return facts


def read_record(path):
    """scratch/plan_shapes.py --compact: "tag dyn setting | mode nw fpb rcap iw tt mcap lds fused slot_width | mode ..."
    -> {tag: facts}, [(tag, mode, dyn, knobs, the nine numbers)]"""
    launches = []
    for line in open(path):
        if line.startswith(("facts ", "#")):
            continue
        head, *modes = line.rstrip("\n").split(" | ")
        tag, dyn, env = head.split(" ", 2)
        knobs = {} if env == "(defaults)" else dict(kv.split("=") for kv in env.split())
        launches += [(tag, m.split()[0], int(dyn), knobs, tuple(int(x) for x in m.split()[1:])) for m in modes]
    return read_facts(path), launches


def plan_in(facts, mode, dyn, knobs, ctx_fuses):
    """F3PlanIn of a recorded launch.  The assignment is asked to fuse by SITATOR_FUSE=1 (mode "fused") unless the call
    maps the lattice dynamically (sit_fill); the context allows it where the record shows a fused pass at all, the call
    has no dynamic mapping and SITATOR_DEBUG_STOP is not set (fill3_launch)."""
    f = dict(facts)
    F = 1000
    f.update(dynmap=dyn, fuse_asked=int(mode == "fused" and not dyn), fuse_ok=int(ctx_fuses and not dyn and int(knobs.get("DEBUG_STOP", 0)) == 0),
             store=int(mode == "plain"), f_lo=0, f_hi=F, F=F, idx_contig=1, idx_s0=0, idx_m0=f["S"], A=f["S"] + f["M"], aligned=1, diag=1, ref_in_cell=1)
    return f


def test_plans_equal_the_recorded_launches_of_the_build_before_the_planner(probe):
    """(a) Every launch of profiles/r08_plan_shapes_parent.txt - C2 to C5 as bench.py builds them, plain, with the
    assignment in kernels of its own and fused, with and without dynamic mapping, under the overrides of
    tests/test_gpu_kernels.py, test_gpu_fill_slots.py and test_gpu_fill_d1e.py: what SITATOR_DEBUG_SHAPE printed and
    sit_info reported (fused, slot width) is what the planner gives."""
    facts, launches = read_record(RECORD)
    assert sorted(facts) == ["C2", "C3", "C4", "C5"] and len(launches) > 500
    fuses = {tag: any(n[7] for t, m, d, k, n in launches if t == tag) for tag in facts}
    assert all(fuses.values())
    cases = [(plan_in(facts[tag], mode, dyn, knobs, fuses[tag]), dict(knobs, FILL_AUTOTUNE=0)) for tag, mode, dyn, knobs, numbers in launches]
    for (tag, mode, dyn, knobs, numbers), got in zip(launches, probe(cases)):
        assert got["err"] is None and tuple(got[k] for k in SHAPE) == numbers, (tag, mode, dyn, knobs)


# S, M, the padded landmark width, W, W_tight, delta >= 0 and the mean candidate counts of C2 - C5: the "facts" lines of
# profiles/r08_plan_shapes_parent.txt (sit_info of the build before the planner); the shapes are that file's "(defaults)"
# lines: plain / SITATOR_FUSE=0 / SITATOR_FUSE=1, each nw fpb rcap iw tt mcap, bytes of LDS, fused, slot width
C2_TO_C5 = {
    "C2": (dict(S=512, M=64, vp=8, W=10, W_tight=6, have_tight=1, mean="7.280451127819549", tight_mean="3.5779220779220777"),
           [(4, 1, 64, 16, 128, 192, 21584, 0, 16), (4, 1, 64, 16, 128, 192, 21584, 0, 16), (4, 1, 64, 16, 128, 192, 21584, 1, 16)]),
    "C3": (dict(S=1088, M=448, vp=8, W=13, W_tight=8, have_tight=1, mean="10.265519096288328", tight_mean="4.212591289514366"),
           [(16, 1, 64, 28, 192, 384, 72752, 0, 0), (16, 1, 64, 28, 192, 384, 72752, 0, 0), (16, 1, 64, 28, 192, 384, 72752, 1, 0)]),
    "C4": (dict(S=2048, M=256, vp=8, W=10, W_tight=6, have_tight=1, mean="7.280451127819549", tight_mean="3.6184719535783367"),
           [(16, 1, 40, 16, 128, 192, 78512, 0, 0), (16, 1, 40, 16, 128, 192, 78512, 0, 0), (8, 1, 64, 32, 192, 320, 74608, 1, 0)]),
    "C5": (dict(S=256, M=160, vp=8, W=35, W_tight=13, have_tight=1, mean="20.953345774460143", tight_mean="8.8593491119180676"),
           [(4, 1, 64, 40, 192, 1408, 21232, 0, 0), (4, 1, 64, 40, 192, 1408, 21232, 0, 0), (4, 1, 64, 40, 192, 1408, 21232, 1, 0)]),
}


@pytest.mark.parametrize("cfg", sorted(C2_TO_C5))
def test_benchmark_configurations_get_the_recorded_shape(probe, cfg):
    """(a), spelled out for the four benchmark configurations with every knob at its default and the autotune off."""
    facts, expected = C2_TO_C5[cfg]
    modes = ("plain", "unfused", "fused")
    got = probe([(plan_in(facts, mode, 0, {}, True), {"FILL_AUTOTUNE": 0}) for mode in modes])
    assert [g["err"] for g in got] == [None] * 3 and [tuple(g[k] for k in SHAPE) for g in got] == expected


def test_autotune_candidates_are_the_recorded_trials(probe):
    """The pairs the autotune times, in order, with their LDS: the "k_fill3 trial:" lines of the parent's run at C2 - C5
    (the winner is a matter of timing and is not compared)."""
    facts = read_facts(RECORD_TUNE)
    trials, tag = {}, None
    for line in open(RECORD_TUNE):
        m = re.match(r"## (\w+) autotune on", line)
        if m:
            tag = m.group(1)
            trials[tag] = []
        m = re.match(r"k_fill3 trial: rcap (\d+) tt (\d+), (\d+) bytes", line)
        if m and tag:
            trials[tag].append(tuple(int(x) for x in m.groups()))
    assert sorted(trials) == ["C2", "C3", "C4", "C5"] and all(trials.values())
    for tag in trials:
        got, = probe([(plan_in(facts[tag], "plain", 0, {}, True), {})])
        assert got["cands"] == trials[tag], tag
        assert got["cands"][0][:2] == (got["rcap"], got["tt"]), "the plan's own pair is tried first"


def grid():
    """inputs around and beyond the benchmark's, with and without a tight table"""
    for S, M in ((512, 64), (1088, 448), (2048, 256), (864, 160), (27, 4), (200, 1), (300, 57), (5000, 30), (100, 3000)):
        for vp in (4, 8, 16):
            for W, W_tight, have_tight in ((20, 8, 1), (20, 8, 0), (70, 33, 1), (9, 9, 1), (255, 100, 1), (64, 64, 0)):
                for dyn in (0, 1):
                    yield dict(S=S, M=M, vp=vp, W=W, W_tight=W_tight, have_tight=have_tight, mean="9.5", tight_mean="4.25", dynmap=dyn, fuse_asked=0,
                               fuse_ok=0, store=1, f_lo=0, f_hi=100, F=100, idx_contig=1, idx_s0=0, idx_m0=S, A=S + M, aligned=1, diag=1, ref_in_cell=1)


def test_knob_overrides_are_honoured_and_clamped(probe):
    """(b) SITATOR_FILL_WAVES is taken if it is 4, 8 or 16; survivor slots in eights up to 64 (and at least a pass of 64 / vp
    tasks); the task table in 64s; windows in fours with at most 4096 candidate tasks; several frames per workgroup only
    with four waves."""
    cases, want = [], []
    for f in grid():
        wmax = max(f["W"], f["W_tight"]) if f["have_tight"] else f["W"]
        for knobs in ({}, {"FILL_WAVES": 4}, {"FILL_WAVES": 8, "FILL_FPB": 2}, {"FILL_WAVES": 16, "FILL_FPB": 3}, {"FILL_WAVES": 5}, {"FILL_FPB": 4},
                      {"FILL_RCAP": 8}, {"FILL_RCAP": 20}, {"FILL_RCAP": 48}, {"FILL_RCAP": 100}, {"FILL_TCAP": 64}, {"FILL_TCAP": 100},
                      {"FILL_TCAP": 1024}, {"FILL_TCAP": 2000}, {"FILL_IW": 4}, {"FILL_IW": 5}, {"FILL_IW": 33}, {"FILL_IW": 64}, {"FILL_IW": 65},
                      {"FILL_WAVES": 4, "FILL_FPB": 4, "FILL_RCAP": 16, "FILL_IW": 33, "FILL_TCAP": 256}):
            cases.append((f, dict(knobs, FILL_AUTOTUNE=0)))
            want.append((f, knobs, wmax))
    for (f, knobs, wmax), p in zip(want, probe(cases)):
        if p["err"]:
            continue
        what = (f, knobs, p["shape"])
        assert p["nw"] in (4, 8, 16) and (knobs.get("FILL_WAVES") not in (4, 8, 16) or p["nw"] == knobs["FILL_WAVES"]), what
        assert p["nw"] == 4 or p["fpb"] == 1, what
        assert 1 <= p["fpb"] <= 32 and p["fpb"] <= max(1, knobs.get("FILL_FPB", 32)), what
        assert p["rcap"] % 8 == 0 and 64 // f["vp"] <= p["rcap"] <= 64, what
        if "FILL_RCAP" in knobs:
            assert p["rcap"] == max(64 // f["vp"], min(64, -(-knobs["FILL_RCAP"] // 8) * 8)) and not p["rcap_auto"], what
        assert p["tt"] % 64 == 0 and 64 <= p["tt"] <= 1024, what
        if 64 <= knobs.get("FILL_TCAP", 0) <= 1024:
            assert p["tt"] == -(-knobs["FILL_TCAP"] // 64) * 64 and not p["tt_auto"], what
        assert p["tt_auto"] == (not 64 <= knobs.get("FILL_TCAP", 0) <= 1024), what
        assert p["iw"] % 4 == 0 and 4 <= p["iw"] <= 64 and (p["iw"] * wmax <= 4096 or p["iw"] == 4), what
        if 1 <= knobs.get("FILL_IW", 0) <= 64:
            iw = -(-knobs["FILL_IW"] // 4) * 4
            while iw > 4 and iw * wmax > 4096:
                iw -= 4
            assert p["iw"] == iw, what
        assert p["mcap"] % 64 == 0 and p["mcap"] >= p["iw"] * wmax, what
        assert p["fpb1"] == (p["fpb"] == 1), what


def test_lds_stays_within_the_limit_or_the_plan_says_why(probe):
    """(c) No plan without an error takes more than 160 KiB - 256 bytes; a frame that does not fit and lists that are too
    long are the two errors."""
    cases = [(f, dict(k, FILL_AUTOTUNE=0)) for f in grid() for k in ({}, {"F3_LDS_PAD": 30000}, {"F3_LDS_PAD": 120000}, {"FILL_FPB": 32}, {"FILL_WAVES": 16, "FILL_RCAP": 64, "FILL_TCAP": 1024, "FILL_IW": 64})]
    plans = probe(cases)
    assert any(p["err"] for p in plans) and any(not p["err"] for p in plans)
    for (f, k), p in zip(cases, plans):
        if p["err"]:
            assert p["err"] == "sit_fill: one frame's atoms do not fit in LDS", (f, k)
        else:
            assert p["lds"] <= LDS_LIMIT and p["lds"] == p["total"] + 32 + k.get("F3_LDS_PAD", 0), (f, k)
            assert all(lds <= 160 * 1024 - 512 for _, _, lds in p["cands"]), (f, k)
    base = next(grid())
    too_big, too_long, fits = probe([(dict(base, S=7000, idx_m0=7000, A=7064), {}), (dict(base, W=20000), {}), (dict(base, S=5400, idx_m0=5400, A=5464), {})])
    assert too_big["err"] == "sit_fill: one frame's atoms do not fit in LDS"             # 7064 atoms x 24 bytes = 169 536
    assert too_long["err"] == "sit_fill: candidate lists too long for the third-generation kernel"      # 4 ions x 20000 > 65536
    # the largest frames fill3_eligible lets through (24 bytes per atom + 8 per ion <= 132 KiB: "room for four waves' tables")
    assert fits["err"] is None and fits["lds"] <= LDS_LIMIT and fits["fpb"] == 1


def test_slot_form_is_chosen_by_its_rule(probe):
    """(d) Possible with one frame per workgroup, no list longer than 64 entries, no dynamic mapping and no ablation stop
    below 10 (the stop counts as 0 under dynamic mapping); the default where four waves meet a primary table without a
    list longer than eight entries; SITATOR_F3_SLOT = 0 / 1 decides where the form is possible."""
    cases = []
    for f in grid():
        for knobs in ({}, {"FILL_WAVES": 4}, {"FILL_WAVES": 8}, {"FILL_WAVES": 16}, {"FILL_FPB": 1}, {"FILL_WAVES": 4, "FILL_FPB": 3}):
            for slot in (None, 0, 1):
                for stop in (0, 3, 9, 10, 12):
                    k = dict(knobs, FILL_AUTOTUNE=0)
                    if slot is not None:
                        k["F3_SLOT"] = slot
                    if stop:
                        k["DEBUG_STOP"] = stop
                    cases.append((f, k))
    seen = set()
    for (f, k), p in zip(cases, probe(cases)):
        if p["err"]:
            continue
        wmax = max(f["W"], f["W_tight"]) if f["have_tight"] else f["W"]
        wprim = f["W_tight"] if f["have_tight"] else f["W"]
        stop = 0 if f["dynmap"] else k.get("DEBUG_STOP", 0)
        assert p["stop"] == stop
        possible = (p["nw"] != 4 or p["fpb"] == 1) and wmax <= 64 and not f["dynmap"] and (stop == 0 or stop >= 10)
        slot = possible and ((p["nw"] == 4 and wprim <= 8) if "F3_SLOT" not in k else k["F3_SLOT"] != 0)
        width = 8
        while width < wmax:
            width *= 2
        assert p["slot"] == int(slot) and p["slot_width"] == (width if slot else 0), (f, k, p["shape"])
        seen.add((bool(possible), bool(slot)))
    assert seen == {(False, False), (True, False), (True, True)}
