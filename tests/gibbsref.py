"""Python twin of the batched posterior sampler of rates (phm_gibbs_rates), written from the spec: a loop of
``samplemodelsref.sample_models(draws=1, replica_offset=i)`` -- section 19's twin, one exact history per evaluation -- plus a
restatement of the conjugate Gamma update with Python's ``math`` functions (Marsaglia & Tsang's squeeze with a Box-Muller normal
over the Philox stream (ENT_RATE | parameter, chain, iteration + replica_offset)).

TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

import pyref
import samplemodelsref

ENT_RATE = 2 << 30


class Stream:
    """sequential uniforms of the stream (seed, entity, iteration word, replica word): draw d is word d & 3 of block d >> 2"""

    def __init__(self, seed, ent, it, rep):
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.ent, self.it, self.rep, self.next, self.blk, self.words = ent, it & 0xFFFFFFFF, rep & 0xFFFFFFFF, 0, -1, None

    def uniform(self):
        d = self.next
        self.next += 1
        if d >> 2 != self.blk:
            self.blk = d >> 2
            self.words = pyref.philox((self.blk, self.ent, self.it, self.rep), self.key)
        return pyref.u01(self.words[d & 3])

    def gamma(self, shape, scale):
        boost = 1.0
        if shape < 1.0:
            u = self.uniform()
            boost = math.pow(u, 1.0 / shape)
            shape += 1.0
        d = shape - 1.0 / 3.0
        c = 1.0 / math.sqrt(9.0 * d)
        while True:
            u1, u2 = self.uniform(), self.uniform()
            z = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
            v = 1.0 + c * z
            if v <= 0.0:
                continue
            v = v * v * v
            u = self.uniform()
            if math.log(u) < 0.5 * z * z + d - d * v + d * math.log(v):
                return d * v * boost * scale


def build_Q(index, theta):
    """Q(theta): q_ij = theta[index - 1], the diagonal minus the row's entries summed left to right"""
    index = np.asarray(index)
    n = index.shape[0]
    Q = np.zeros((n, n))
    for i in range(n):
        row = 0.0
        for j in range(n):
            if j != i and index[i, j] > 0:
                Q[i, j] = float(theta[index[i, j] - 1])
                row += Q[i, j]
        Q[i, i] = -row
    return Q


def update(index, theta, stats_by_site, prior, theta_max, seed, chain, rep):
    """One chain's Gamma update from its histories' statistics, stats_by_site [S_eval, n + n(n-1)] (sites ascending).  Returns
    (theta', rejected [p])."""
    index = np.asarray(index)
    n = index.shape[0]
    theta = np.array(theta, dtype=np.float64)
    rej = np.zeros(theta.size, dtype=np.int64)
    for c in range(theta.size):
        Nc = Wc = 0.0
        for row in np.atleast_2d(stats_by_site):
            for i in range(n):
                for j in range(n):
                    if i != j and index[i, j] == c + 1:
                        Nc += float(row[n + i * (n - 1) + (j - 1 if j > i else j)])
                        Wc += float(row[i])
        fresh = Stream(seed, ENT_RATE | c, chain, rep).gamma(float(prior[c][0]) + Nc, 1 / (float(prior[c][1]) + Wc))
        if fresh > theta_max or not fresh > 0.0:
            rej[c] += 1
        else:
            theta[c] = fresh
    return theta, rej


def run(edge, edge_length, index, theta0, prior, theta_max, pid, sites, iters, observe=None, site_of_chain=None, thin=1, seed=0,
        replica_offset=0):
    """The whole driver: theta [rows, C, p], loglik [rows, C], stats [rows, C, cols], rejected [C, p], status [C]."""
    index = np.asarray(index)
    n = index.shape[0]
    theta = np.array(theta0, dtype=np.float64)
    Cn, p = theta.shape
    prior = np.asarray(prior, dtype=np.float64)
    if prior.ndim == 2:
        prior = np.broadcast_to(prior, (Cn,) + prior.shape)
    sites = np.atleast_2d(np.asarray(sites))
    cols = n + n * (n - 1)
    rows = -(-iters // thin)
    out_t, out_l, out_s = np.full((rows, Cn, p), np.nan), np.full((rows, Cn), np.nan), np.full((rows, Cn, cols), np.nan)
    rejected, status = np.zeros((Cn, p), dtype=np.int64), np.zeros(Cn, dtype=np.int64)
    for i in range(iters):
        Qs = np.stack([build_Q(index, t) for t in theta])
        r = samplemodelsref.sample_models(edge, edge_length, Qs, pid, sites, 1, observe=observe, site_of_model=site_of_chain,
                                          seed=seed, replica_offset=i + replica_offset)
        st = r["stats"][..., 0, :].reshape(Cn, -1, cols)                   # [C, S_eval, cols]
        ll = r["loglik"].reshape(Cn, -1)
        for k in range(Cn):
            tot = 0.0
            for v in ll[k]:
                tot += float(v)
            if not math.isfinite(tot):
                status[k] = 1
            if status[k]:
                continue
            if i % thin == 0:
                out_t[i // thin, k], out_l[i // thin, k] = theta[k], tot
                acc = np.zeros(cols)
                for row in st[k]:
                    acc = acc + row
                out_s[i // thin, k] = acc
            theta[k], rej = update(index, theta[k], st[k], prior[k], theta_max, seed, k, i + replica_offset)
            rejected[k] += rej
    return dict(theta=out_t, loglik=out_l, stats=out_s, rejected=rejected, status=status)
