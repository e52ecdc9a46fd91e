"""The pure host pieces of the exact samplers' tile driver and of the wide tree passes' device state
(phylomap_amd/csrc/phm_sample_host.h and phm_ancestral_wide_host.h, DESIGN.md sections 19b and 23a) without a device: the wide
chunk plan -- with the fallback that shrinks the sites of a chunk when not even one model fits with all of them, and its floor of
one site, which no GPU test reaches on a card of this size --, the tiles of an evaluation and the scatter of a flushed batch.  A
stand-alone program (tests/native/sample_host_check.cpp) is built with hipcc and AddressSanitizer + UBSan on the host side, run on
its own, and its output compared with a direct transcription of the formulas and plain loops that aw_device and sw_device had
before they shared this code."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AW_GRID_MAX = 65535
SW_ITEMS_MAX = 1 << 30
SM_TILE = 32                                            # sizeof(phm::SmTile)
T, NN_, E, NT, S, J, D, DEPTH = 6, 5, 10, 11, 1000, 5, 70, 20
FREES = (0, 1 << 20, 4190288, 21157808, 1 << 28, 64 << 30)


def lanes(n):
    return 16 if n <= 16 else 32 if n <= 32 else 64


def ancestral_plan(free_b, n, paired, count, chunk):
    """aw_device's chunk arithmetic as it stood, marginal and joint asked for"""
    nn, NP, Nn = n * n, lanes(n), NN_
    work_b = 8 * 5 * nn * E
    budget = free_b // 2 - work_b if free_b // 2 > work_b else 0
    per_model = 8 * (E * nn + nn + n) + 4 * E + 4 + (T if paired else 0)
    per_eval = (8 * NP + 4) * NT + 8
    per_eval += (8 * NP + 4) * NT + 8 * J * n
    per_eval += (8 * NP + 4) * Nn + E * NP + NT + 8
    S_eval = 1 if paired else S
    Sc_max = min(S_eval, AW_GRID_MAX)
    Kc_max = budget // (per_model + per_eval * Sc_max)
    if Kc_max < 1:
        Kc_max = 1
        Sc_max = max(1, min(Sc_max, (budget - per_model) // per_eval if budget > per_model else 1))
    step_max = AW_GRID_MAX
    if chunk > 0:
        Kc_max, Sc_max, step_max = min(Kc_max, chunk), min(Sc_max, chunk), min(step_max, chunk)
    Kc_max = min(Kc_max, count, AW_GRID_MAX)
    return Kc_max, Sc_max, step_max


def sampler_plan(free_b, n, paired, count, chunk):
    """sw_device's tile count and chunk arithmetic as it stood, node states asked for; None: its PHM_ERR_CAPACITY return"""
    nn, NP, cols = n * n, lanes(n), n + n * (n - 1)
    S_eval = 1 if paired else S
    tab_b = 8 * (DEPTH + 1) * nn
    work_b = 8 * 5 * nn * E
    per_tile = NT * 64 + 64 * (8 * (cols + n) + 4 * n * (n - 1)) + 4 * 64 * NT + SM_TILE
    tiles_total = count * S_eval * ((D + 63) // 64)
    Tc_max = max(1, min(tiles_total, free_b // 8 // per_tile, 1 << 20, SW_ITEMS_MAX // E))
    if chunk > 0:
        Tc_max = min(Tc_max, chunk)
    fixed_b = work_b + per_tile * Tc_max
    budget = free_b // 2 - fixed_b if free_b // 2 > fixed_b else 0
    per_model = 8 * (E * nn + 2 * nn + n + 1) + 4 * (E + 1) + 4 + (T if paired else 0) + tab_b
    per_eval = (8 * NP + 4) * NT + 8
    if budget < per_model + per_eval:
        return per_tile, Tc_max, None
    Sc_max = min(S_eval, AW_GRID_MAX)
    Kc_max = budget // (per_model + per_eval * Sc_max)
    if Kc_max < 1:
        Kc_max = 1
        Sc_max = max(1, min(Sc_max, (budget - per_model) // per_eval))
    step_max = AW_GRID_MAX
    if chunk > 0:
        Kc_max, Sc_max, step_max = min(Kc_max, chunk), min(Sc_max, chunk), min(step_max, chunk)
    Kc_max = min(Kc_max, count, AW_GRID_MAX)
    return per_tile, Tc_max, (Kc_max, Sc_max, step_max)


def expected_output():
    lines = []
    seen = {(who, n): set() for who in ("ancestral", "sampler") for n in (9, 64)}
    for n in (9, 64):
        for paired in (0, 1):
            for free_b in FREES:
                for chunk in (0, 1, 100):
                    for count in (1, 3, 130):
                        tail = f"n={n} paired={paired} free={free_b} chunk={chunk} count={count} ->"
                        kc, sc, step = ancestral_plan(free_b, n, paired, count, chunk)
                        lines.append(f"ancestral {tail} Kc_max={kc} Sc_max={sc} step_max={step}")
                        if chunk == 0 and not paired:
                            seen["ancestral", n].add("ample" if sc == S else "shrunk" if sc > 1 else "one")
                        per_tile, tc, pl = sampler_plan(free_b, n, paired, count, chunk)
                        head = f"sampler per_tile={per_tile} Tc_max={tc} "
                        if pl is None:
                            lines.append(head + f"{tail} capacity")
                        else:
                            lines.append(head + f"plan {tail} Kc_max={pl[0]} Sc_max={pl[1]} step_max={pl[2]}")
                            if chunk == 0 and not paired:
                                seen["sampler", n].add("ample" if pl[1] == S else "shrunk" if pl[1] > 1 else "one")
                        if paired:                      # one site per model: nothing to shrink
                            assert sc == 1 and (pl is None or pl[1] == 1)
    # at 9 and at 64 states the cross-mode grid reaches all three regimes: all sites fit, sites shrunk, one site (the sampler
    # refuses with PHM_ERR_CAPACITY where not even one evaluation fits, so it has no floor to reach)
    for n in (9, 64):
        assert seen["ancestral", n] == {"ample", "shrunk", "one"}, seen
        assert {"ample", "shrunk"} <= seen["sampler", n], seen
    for draws in (3, 64, 70, 129):
        ev, h_first = 7, 2 * draws
        for d0 in range(0, draws, 64):                  # the loop of sm_device and sw_device
            lines.append(f"tile D={draws} ev=5 k=2 eval_id=77 d0={d0} n_valid={min(64, draws - d0)} pad=0 row0={ev * draws + d0 - h_first}")
    cols, NTs, H, h_first = 3, 4, 4 * D, D
    tiles = [(ev * D + d0 - h_first, min(64, D - d0)) for ev in (1, 3) for d0 in range(0, D, 64)]
    nt = len(tiles)
    npad = nt * 64
    outh = [1000 + i for i in range(cols * npad)]
    nodes_h = [5000 + i for i in range(npad * NTs)]
    stats, nodes = [-1] * (cols * H), [-1] * (H * NTs)
    for i, (row0, nv) in enumerate(tiles):              # flush()'s plain loops
        h0 = h_first + row0
        for c in range(cols):
            stats[h0 + H * c:h0 + H * c + nv] = outh[c * npad + i * 64:c * npad + i * 64 + nv]
        nodes[h0 * NTs:(h0 + nv) * NTs] = nodes_h[i * 64 * NTs:(i * 64 + nv) * NTs]
    assert [nv for _, nv in tiles] == [64, 6, 64, 6] and stats.count(-1) == cols * 2 * D
    lines.append("stats " + " ".join(str(v) for v in stats))
    lines.append("nodes " + " ".join(str(v) for v in nodes))
    lines.append("stats alone equal")
    lines.append("ok")
    return lines


def test_plan_tiles_and_scatter_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "sample_host_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "sample_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got, want = run.stdout.splitlines(), expected_output()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
