"""Python twin of the MCMC stochastic maps: pyref.sumstatMCMC restated so that it records, at the
iterations ``map_iters``, every branch's path after the interior states are resampled and equal neighbours merged, before the
virtual jumps go back in -- ``(nd, ns)`` of pyref's branch step.  Built from pyref's primitives (streams, chains, categorical
rule); packed in the library's layout with mapsref._pack: history ``h = s * J + j`` is chain s at ``map_iters[j]``, row
``h * E + b`` its map on edge row b.
TEST INFRASTRUCTURE ONLY.
"""
import mapsref
import pyref
from pyref import ENT_BEXP, ENT_BSTATE, ENT_NODE


def sumstatMCMC(z, Q, pid, Omega, N, nen, nodelist, root, seed, replica, variant="plain", map_iters=None):
    """pyref.sumstatMCMC for one chain with the merged paths recorded: (out, rows), rows[(j, b)] = [(dwell, state0), ...] for
    the j-th recorded iteration (map_iters; None: every iteration).  ``out`` is pyref's, from the same numbers in the same order."""
    n = len(Q)
    E = len(z["edge"])
    T = len(z["states"])
    rec = {it: j for j, it in enumerate(range(N) if map_iters is None else map_iters)}
    e1 = [int(r[0]) for r in z["edge"]]
    e2 = [int(r[1]) for r in z["edge"]]
    B2 = [[(1.0 if i == j else 0.0) + Q[i][j] / Omega for j in range(n)] for i in range(n)]
    Bc = [[(b if b > 1e-7 else 0.0) for b in row] for row in B2] if variant == "sparse" else B2
    rng = pyref.Rng(seed, replica)
    dw = [[float(x) for x in z["maps"][b]] for b in range(E)]
    st = [[int(x) - 1 for x in z["mapnames"][b]] for b in range(E)]
    PL = [[0.0] * n for _ in range(2 * T - 1)]
    hid = variant == "ks"
    ks = hid or variant == "bf"
    kk = n // 2 - 1 if hid else 0
    for i in range(T):
        if not hid:
            PL[i][int(z["states"][i]) - 1] = 1.0
        else:
            for j in range(1 if int(z["states"][i]) % 2 == 0 else 0, n, 2):
                PL[i][j] = 1.0
    cols = n + n * n + 2 + 3 * kk + 1 if ks else n + n * (n - 1)
    out = [[0.0] * cols for _ in range(N)]
    rows = {}
    for it in range(N):
        if ks:
            base = n + n * n
            out[it][base], out[it][base + 1] = Q[0][1], Q[1][0]
            for i in range(kk):
                out[it][base + 2 + i] = Q[2 * i][2 * i + 2]
                out[it][base + 2 + kk + i] = Q[2 * i + 2][2 * i]
                out[it][base + 2 + 2 * kk + i] = Q[2 * (i + 1)][2 * (i + 1) + 1] / Q[0][1]
        m = [len(d) for d in dw]
        for i in range(T - 1):
            ea, eb = nen[2 * i] - 1, nen[2 * i + 1] - 1
            first = list(PL[e2[eb] - 1])
            second = list(PL[e2[ea] - 1])
            for _ in range(m[eb] - 1):
                first = pyref.matvec(Bc, first)
            for _ in range(m[ea] - 1):
                second = pyref.matvec(Bc, second)
            row = [first[c] * second[c] for c in range(n)]
            if variant == "bigtree" or ks:
                s = pyref.rowsum(row)
                row = [x / s for x in row]
            PL[e1[ea] - 1] = row
        rm = [0] * (2 * T - 1)
        for i in range(T):
            rm[i] = int(z["states"][i]) - 1
        rm[root - 1] = pyref.sample([pid[c] * PL[root - 1][c] for c in range(n)], rng.u(it, ENT_NODE | (root - 1), 0))
        for node in nodelist:
            j = e2.index(node)
            ps = rm[e1[j] - 1]
            v = [0.0] * n
            v[ps] = 1.0
            for _ in range(m[j] - 1):
                v = pyref.matTvec(Bc, v)
            rm[node - 1] = pyref.sample([v[c] * PL[node - 1][c] for c in range(n)], rng.u(it, ENT_NODE | (node - 1), 0))
        if ks:
            out[it][cols - 1] = float(rm[root - 1])
        if hid:
            for b in range(E):
                if e2[b] <= T:
                    ps = rm[e1[b] - 1]
                    v = [0.0] * n
                    v[ps] = 1.0
                    for _ in range(m[b] - 1):
                        v = pyref.matTvec(Bc, v)
                    rm[e2[b] - 1] = pyref.sample([v[c] * PL[e2[b] - 1][c] for c in range(n)], rng.u(it, ENT_NODE | (e2[b] - 1), 0))
        for b in range(E):
            st[b][0] = rm[e1[b] - 1]
            st[b][-1] = rm[e2[b] - 1]
        for b in range(E):
            ss = len(dw[b])
            if ss > 2:
                beta = [[0.0] * n]
                beta[0][st[b][-1]] = 1.0
                for j in range(1, ss - 1):
                    beta.append(pyref.matvec(Bc, beta[j - 1]))
                for i in range(1, ss - 1):
                    p = [B2[st[b][i - 1]][c] * beta[ss - i - 1][c] for c in range(n)]
                    st[b][i] = pyref.sample(p, rng.u(it, ENT_BSTATE | b, i - 1))
            if ks:
                for i in range(1, ss):
                    out[it][n + st[b][i - 1] * n + st[b][i]] += 1.0
            nd, ns = [dw[b][0]], [st[b][0]]
            for i in range(1, ss):
                if st[b][i] != ns[-1]:
                    nd.append(dw[b][i]); ns.append(st[b][i])
                else:
                    nd[-1] = nd[-1] + dw[b][i]
            if it in rec:                                                    # the map: (nd, ns) of this branch step
                rows[(rec[it], b)] = list(zip(nd, ns))
            for i in range(1, len(ns)):
                a, c = ns[i - 1], ns[i]
                if not ks:
                    out[it][n + a * (n - 1) + (c - 1 if a < c else c)] += 1.0
            fd, fs, ed = [], [], 0
            for seglen, s in zip(nd, ns):
                scale = 1.0 / (Omega + Q[s][s])
                tot = 0.0
                while tot < seglen:
                    rl = scale * rng.e(it, ENT_BEXP | b, ed)
                    ed += 1
                    if tot + rl < seglen:
                        fd.append(rl); fs.append(s); tot += rl
                    else:
                        fd.append(seglen - tot); fs.append(s); tot = seglen
            dw[b], st[b] = fd, fs
        for b in range(E):
            for d, s in zip(dw[b], st[b]):
                out[it][s] += d
    return out, rows


def pack(chain_rows, J, E):
    """[rows of chain 0, rows of chain 1, ...] (each from sumstatMCMC) -> (off, dwell, state), history s * J + j"""
    rows = {}
    for s, rws in enumerate(chain_rows):
        for (j, b), segs in rws.items():
            rows[(s * J + j, b)] = segs
    return mapsref._pack(rows, len(chain_rows) * J, E)


def history(chain_rows_one, j, E):
    """one history's rows as (off, dwell, state) -- compare with a Maps row block"""
    return mapsref._pack({(0, b): chain_rows_one[(j, b)] for b in range(E)}, 1, E)
