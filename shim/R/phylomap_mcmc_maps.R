# Stochastic maps of the MCMC samplers on the GPU (shim/phylomap_mcmc_maps_shim.cpp -> phm_maketreelistMCMC_maps): the fixed-Q
# samplers sumstatMCMC, sumstatMCMC_bigtree, SPARSEsumstatMCMC and the fixed-Q sweeps of sumstatMCMCks / sumstatMCMCbf, with the
# chains' sampled histories at chosen iterations.  set.seed() controls the result; the phylomap.hip.* options of
# phylomap_hip_options.R apply (replicas, reduce, device, devices, rescale, mapping, cap_tail).  Drop this file into the package's
# R/ directory next to phylomap_maps.R, whose history_tree() reads the maps.
#
# map_iters: rows of the statistics matrix (1-based, increasing) whose histories are kept; NULL keeps every row.  History
# h = (s - 1) * J + j (1-based j over map_iters, s over chains) is chain s at row map_iters[j].
# variant: "plain" (sumstatMCMC), "bigtree", "sparse", "ks" (hidden rates, Q fixed) or "bf" (Q fixed).
# Returns list(stats, maps): stats as the plain sampler returns them, maps = list(off, dwell, state, n_hist, n_edge).
sumstatMCMCmaps <- function(z, Q, pid, Omega, N, map_iters = NULL, variant = "plain") {
  its <- if (is.null(map_iters)) integer(0) else as.integer(map_iters) - 1L
  .Call('phylomap_hip_mcmc_maps', PACKAGE = 'phylomap', z, Q, as.numeric(pid), as.numeric(Omega), as.integer(N), its,
        as.character(variant))
}
