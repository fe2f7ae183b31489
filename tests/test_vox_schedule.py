"""CPU tier: vox_schedule (csrc/lvi_vox_schedule.hpp), the one function that decides which launches a run of the VoxelGrid
consists of.  A stand-alone driver is compiled with g++ against that header alone (it includes nothing from HIP), fed EVERY
combination of the VoxPlanState fields for 1, 2 and 3 slots, and compared with an independent restatement of the rules:

  * the mode is SORTED as soon as one slot resolves SORTED; sorted with more than one slot runs slot by slot;
  * WITH_PLAN / DET_PER_RUN iff the mode is BINNED and every slot is per-run and owns the tables;
  * otherwise the bbox is CACHED iff every slot's bbox records are valid, else MINMAX;
  * in BINNED mode DET_CACHED iff every slot's bbox records and counts are valid, else RESERVE; NONE when sorted;
  * fold_slots iff S > 1 and every plan is slot-major with host-known lengths."""
import os
import subprocess

import numpy as np
import pytest

SORTED, BINNED = 1, 2
MINMAX, CACHED, WITH_PLAN = 0, 1, 2
NONE, RESERVE, DET_CACHED, DET_PER_RUN = 0, 1, 2, 3
FIELDS = ("mode", "det_tables", "per_run", "bbox_valid", "counts_valid", "n_host", "slot_major")

DRIVER = r"""
#include "lvi_vox_schedule.hpp"
#include <cstdio>
using namespace lvi;
static_assert(VOX_SORTED == 1 && VOX_BINNED == 2, "modes");
static_assert(VOX_BBOX_MINMAX == 0 && VOX_BBOX_CACHED == 1 && VOX_BBOX_WITH_PLAN == 2, "bbox sources");
static_assert(VOX_PART_NONE == 0 && VOX_PART_RESERVE == 1 && VOX_PART_DET_CACHED == 2 && VOX_PART_DET_PER_RUN == 3, "partitions");
static void row(const VoxSchedule& s, bool binary)
{
    const unsigned char b[6] = {(unsigned char)s.mode, (unsigned char)s.bbox, (unsigned char)s.part, (unsigned char)s.fold_slots, (unsigned char)s.slot_by_slot, (unsigned char)s.key()};
    if (binary) fwrite(b, 1, 6, stdout);
    else printf("%d %d %d %d %d %d\n", b[0], b[1], b[2], b[3], b[4], s.key());
}
static VoxPlanState unpack(int c)     // bit 0: BINNED (else SORTED); bits 1..6: the six flags in declaration order
{
    return VoxPlanState{(c & 1) ? VOX_BINNED : VOX_SORTED, (c & 2) != 0, (c & 4) != 0, (c & 8) != 0, (c & 16) != 0, (c & 32) != 0, (c & 64) != 0};
}
int main(int argc, char** argv)
{
    if (argc > 1) {
        // every combination for S slots, slot z's state = digit z of the row number in base 128; 6 bytes per row
        const int S = argv[1][0] - '0';
        long rows = 1;
        for (int z = 0; z < S; z++) rows *= 128;
        for (long i = 0; i < rows; i++) {
            VoxPlanState st[3];
            long r = i;
            for (int z = 0; z < S; z++) { st[z] = unpack((int)(r % 128)); r /= 128; }
            row(vox_schedule(st, S), true);
        }
        return 0;
    }
    // stdin: one batch per line: S, then S states as 7 integers each (mode, then the six flags in declaration order)
    int S;
    while (scanf("%d", &S) == 1) {
        VoxPlanState st[3];
        for (int z = 0; z < S; z++) {
            int v[7];
            for (int k = 0; k < 7; k++) if (scanf("%d", &v[k]) != 1) return 2;
            st[z] = VoxPlanState{v[0], v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0};
        }
        row(vox_schedule(st, S), false);
    }
    return 0;
}
"""


def state(mode=BINNED, det_tables=False, per_run=False, bbox_valid=False, counts_valid=False, n_host=False, slot_major=True):
    return (mode, int(det_tables), int(per_run), int(bbox_valid), int(counts_valid), int(n_host), int(slot_major))


def raw_map(mode=BINNED, cache=False, bbox=False, counts=False):
    """a slot of the raw local map as stage_map_build describes it: per-run by default, cached under map_plan_cache"""
    return state(mode, det_tables=True, per_run=not cache, bbox_valid=cache and bbox, counts_valid=cache and counts, n_host=True)


def rules(batch):
    """the rules of the module docstring, restated without looking at the header's code"""
    st = [dict(zip(FIELDS, s)) for s in batch]
    S = len(st)
    mode = SORTED if any(s["mode"] == SORTED for s in st) else BINNED
    if mode == BINNED and all(s["per_run"] and s["det_tables"] for s in st):
        bbox, part = WITH_PLAN, DET_PER_RUN
    else:
        bbox = CACHED if all(s["bbox_valid"] for s in st) else MINMAX
        if mode == SORTED:
            part = NONE
        else:
            part = DET_CACHED if all(s["bbox_valid"] and s["counts_valid"] for s in st) else RESERVE
    fold = S > 1 and all(s["slot_major"] and s["n_host"] for s in st)
    return (mode, bbox, part, int(fold), int(mode == SORTED and S > 1))


@pytest.fixture(scope="module")
def schedule(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("vox_schedule")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", str(exe), str(d / "driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr

    def run(batches):
        text = "".join("%d %s\n" % (len(b), " ".join(str(v) for s in b for v in s)) for b in batches)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        rows = [tuple(int(v) for v in ln.split()) for ln in out.stdout.splitlines()]
        assert len(rows) == len(batches)
        return rows
    run.exe = str(exe)
    return run


@pytest.mark.parametrize("S", [1, 2, 3])
def test_every_combination_of_the_state_fields(schedule, S):
    """128 states per slot: 128, 16 384 and 2 097 152 batches, enumerated by the driver and, in the same order, by numpy"""
    raw = subprocess.run([schedule.exe, str(S)], capture_output=True)
    assert raw.returncode == 0
    got = np.frombuffer(raw.stdout, np.uint8).reshape(-1, 6)
    assert len(got) == 128 ** S
    code = (np.arange(128 ** S)[:, None] // 128 ** np.arange(S)[None, :]) % 128                  # [row, slot]
    f = {name: (code >> k & 1).astype(bool) for k, name in enumerate(FIELDS)}
    sorted_ = (~f["mode"]).any(1)                                                               # bit 0 clear: the slot resolved SORTED
    per_run = ~sorted_ & (f["per_run"] & f["det_tables"]).all(1)
    bbox_all = f["bbox_valid"].all(1)
    counts_all = (f["bbox_valid"] & f["counts_valid"]).all(1)
    want = np.zeros_like(got[:, :5])
    want[:, 0] = np.where(sorted_, SORTED, BINNED)
    want[:, 1] = np.where(per_run, WITH_PLAN, np.where(bbox_all, CACHED, MINMAX))
    want[:, 2] = np.where(per_run, DET_PER_RUN, np.where(sorted_, NONE, np.where(counts_all, DET_CACHED, RESERVE)))
    want[:, 3] = (f["slot_major"] & f["n_host"]).all(1) & (S > 1)
    want[:, 4] = sorted_ & (S > 1)
    bad = np.flatnonzero((got[:, :5] != want).any(1))
    assert len(bad) == 0, (code[bad[0]], got[bad[0]], want[bad[0]])
    # the key tells every schedule apart
    packed = np.unique(got[:, :5].astype(np.int64) @ (8 ** np.arange(5)) * 256 + got[:, 5])
    assert len(np.unique(packed % 256)) == len(packed)


def test_numpy_rules_agree_with_the_scalar_restatement(schedule):
    """the two restatements of this file say the same on a sample the scalar one can afford"""
    rng = np.random.default_rng(3)
    batches = [tuple(state(*((BINNED if c & 1 else SORTED,) + tuple(bool(c >> k & 1) for k in range(1, 7)))) for c in rng.integers(0, 128, S))
               for S in (1, 2, 3) for _ in range(300)]
    for b, row in zip(batches, schedule(batches)):
        assert row[:5] == rules(b), (b, row)


def test_named_cases(schedule):
    ring = state(BINNED)                                            # generic plans: ring, scan (device lengths) …
    submap = state(BINNED, n_host=True)                             # … depth, Submap (host lengths)
    cases = [
        ("default raw map, binned", (raw_map(),), (BINNED, WITH_PLAN, DET_PER_RUN, 0, 0)),
        ("default raw map, 3 slots", (raw_map(),) * 3, (BINNED, WITH_PLAN, DET_PER_RUN, 1, 0)),
        ("default raw map resolved sorted", (raw_map(SORTED),), (SORTED, MINMAX, NONE, 0, 0)),
        ("cached, both valid", (raw_map(cache=True, bbox=True, counts=True),), (BINNED, CACHED, DET_CACHED, 0, 0)),
        ("cached, first build under AUTO", (raw_map(SORTED, cache=True, bbox=True),), (SORTED, CACHED, NONE, 0, 0)),
        ("cached, bbox valid, counts not yet", (raw_map(cache=True, bbox=True),), (BINNED, CACHED, RESERVE, 0, 0)),
        ("cached, nothing valid", (raw_map(cache=True),), (BINNED, MINMAX, RESERVE, 0, 0)),
        ("generic, binned", (ring,), (BINNED, MINMAX, RESERVE, 0, 0)),
        ("generic with host lengths, binned", (submap,), (BINNED, MINMAX, RESERVE, 0, 0)),
        ("generic, sorted", (state(SORTED),), (SORTED, MINMAX, NONE, 0, 0)),
        ("generic batch (device lengths never fold)", (ring,) * 3, (BINNED, MINMAX, RESERVE, 0, 0)),
        ("one slot of three sorted", (raw_map(), raw_map(SORTED), raw_map()), (SORTED, MINMAX, NONE, 1, 1)),
        ("mixed batch", (raw_map(), raw_map(cache=True, bbox=True, counts=True)), (BINNED, MINMAX, RESERVE, 1, 0)),
        ("mixed batch, other order", (raw_map(cache=True, bbox=True, counts=True), raw_map(), raw_map()), (BINNED, MINMAX, RESERVE, 1, 0)),
    ]
    got = schedule([c[1] for c in cases])
    for (name, _, want), row in zip(cases, got):
        assert row[:5] == want, name


def test_fold_slots_needs_every_plan_slot_major_with_host_lengths(schedule):
    ok = raw_map()
    not_major = state(BINNED, det_tables=True, per_run=True, n_host=True, slot_major=False)
    no_lengths = state(BINNED, det_tables=True, per_run=True, n_host=False)
    batches = [(ok,), (ok, ok), (ok, ok, ok)]
    batches += [tuple(bad if z == i else ok for z in range(3)) for bad in (not_major, no_lengths) for i in range(3)]
    got = schedule(batches)
    assert [r[3] for r in got] == [0, 1, 1] + [0] * 6
    assert all(r[:3] == (BINNED, WITH_PLAN, DET_PER_RUN) for r in got)
