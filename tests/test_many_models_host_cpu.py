"""The pure host pieces of the many-model core (phylomap_amd/csrc/phm_loglik_host.h) without a device: the
chunk plan -- with the fallback that shrinks the sites of a chunk when not even 64 models fit, which no GPU test reaches on a card
of this size -- and the staging of models and tips.  A stand-alone program (tests/native/many_models_host_check.cpp) is built with
hipcc and AddressSanitizer + UBSan on the host side, run on its own, and its output compared with a direct transcription of the
formulas and plain loops the drivers had before they shared this code."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_WORK = 256 << 20
LL_REG_MAX = 4                                          # phm_loglik.h: up to 4 states P is built in registers


def plan(free_b, n, paired, S, count, chunk, fixed, pm_extra, pe_extra, T=6, E=10, NT=11):
    """ll_lanes_device's chunk arithmetic as it stood in every driver, the caller's terms added to the sums"""
    nn = n * n
    ws = n > LL_REG_MAX
    fixed = fixed + (LL_WORK if ws else 0)
    budget = free_b // 2 - fixed if free_b // 2 > fixed else 0
    per_model = 8 * (E * nn + nn + n) + 4 + pm_extra
    per_eval = 8 * (NT * (n + 1) + 1) + (T if paired else 0) + pe_extra
    S_eval = 1 if paired else S
    Sc_max = min(S_eval, 65535)
    Kc_max = budget // (per_model + per_eval * Sc_max) // 64 * 64
    if Kc_max < 64:
        Kc_max = 64
        per64 = budget // 64
        Sc_max = max(1, min(Sc_max, (per64 - per_model) // per_eval if per64 > per_model else 1))
    if chunk > 0:
        Kc_max = min(Kc_max, (chunk + 63) // 64 * 64)
        Sc_max = min(Sc_max, chunk)
    Kc_max = min(Kc_max, (count + 63) // 64 * 64)
    ne_max = E
    if ws:
        ne_max = max(1, min(E, 65535, LL_WORK // (8 * 4 * nn * Kc_max)))
    ne_max = min(ne_max, 65535)
    if chunk > 0:
        ne_max = min(ne_max, chunk)
    return Kc_max, Sc_max, ne_max


def expected_output():
    lines = []
    seen = {3: set(), 5: set()}
    for n in (3, 5):
        for paired in (0, 1):
            for x in ((0, 0, 0), (4096, 100, 50)):
                for free_b in (0, 1 << 20, 2 * LL_WORK + (1 << 20), 64 << 30):
                    for chunk in (0, 2, 100):
                        for count in (1, 64, 65, 130):
                            kc, sc, ne = plan(free_b, n, paired, 1000, count, chunk, *x)
                            lines.append(f"plan n={n} paired={paired} extra={x[0]},{x[1]},{x[2]} free={free_b} chunk={chunk} "
                                         f"count={count} -> Kc_max={kc} Sc_max={sc} ne_max={ne}")
                            if chunk == 0 and not paired:
                                seen[n].add("ample" if sc == 1000 else "shrunk" if sc > 1 else "one")
                            if paired:                  # one site per model: the fallback runs (Kc_max = 64) but has nothing to shrink
                                assert sc == 1
    # at 3 and at 5 states the cross-mode grid reaches the fallback that shrinks the sites, and past it the floor of one site
    assert seen == {3: {"ample", "shrunk", "one"}, 5: {"ample", "shrunk", "one"}}, seen
    K, T, S, nn = 70, 5, 5, 9
    tips = [[(s * 7 + t * 3) % 4 for t in range(T)] for s in range(S)]
    owner = [(k * 37 + 11) % S for k in range(K)]
    assert sorted(set(owner)) == list(range(S)) and owner != sorted(owner)
    Qr = [i // nn * 100 + i % nn for i in range(K * nn)]
    for m0, Kc in ((0, 64), (64, 6), (0, 70)):
        Kp = (Kc + 63) // 64 * 64
        Qh = [0] * (nn * Kp)
        th = [0] * (T * Kp)
        for k in range(Kc):                             # the plain loops
            for e in range(nn):
                Qh[e * Kp + k] = Qr[(m0 + k) * nn + e]
            y = tips[owner[m0 + k]]
            for t in range(T):
                th[t * Kp + k] = y[t]
        lines.append(f"models m0={m0} Kc={Kc} Kp={Kp} {len(Qh)}" +
                     "".join((" | " if i % Kp == 0 else " ") + str(v) for i, v in enumerate(Qh)))
        lines.append(f"paired m0={m0} Kc={Kc} tips {len(th)}" + "".join((" | " if i % Kp == 0 else "") + str(v) for i, v in enumerate(th)))
    th = [tips[2 + s][t] for s in range(3) for t in range(T)]
    lines.append(f"cross s0=2 Sc=3 tips {len(th)}" + "".join((" | " if i % T == 0 else "") + str(v) for i, v in enumerate(th)))
    lines.append("ok")
    return lines


def test_plan_and_staging_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "many_models_host_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "many_models_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got, want = run.stdout.splitlines(), expected_output()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
