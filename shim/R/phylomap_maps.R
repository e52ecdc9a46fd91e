# Stochastic maps of simulated and sampled histories on the GPU (shim/phylomap_maps_shim.cpp -> phm_simulate_histories_maps,
# phm_maketreelistEXP_maps): the histories themselves, one map per (history, edge row), and the tree of one history in the shape
# divtophy / nodestatesmake / makemappededge give it (R/sourceme.R:1-60).  set.seed() controls the result.  Drop this file into
# the package's R/ directory next to phylomap_simulate.R.
#
# A maps value is list(off, dwell, state, n_hist, n_edge): row k = r * n_edge + b (0-based) is history r's map on edge row b,
# segments off[k + 1] + 1 .. off[k + 2] (R's 1-based indexing) of dwell (time) and state (1-based), parent end first.

# R forward simulations: list(tips, stats, nodes, maps) -- tips / stats / nodes as simulate_histories() returns them; the maps hold
# TRUE states (what `observe` reports only changes tips).
simulate_maps <- function(tree, Q, pid, R = 1, observe = NULL) {
  obs <- if (is.null(observe)) integer(0) else as.integer(observe)
  .Call('phylomap_hip_simulate_maps', PACKAGE = 'phylomap', tree, Q, as.numeric(pid), as.integer(R), obs)
}

# sumstatEXP (R/sumstatEXP.R:21-33) that also returns its N i.i.d. histories: list(stats = N x (n + n(n-1)), maps).
# options(phylomap.hip.rescale = TRUE) rescales the pruning pass (needed beyond a few hundred tips).
sumstatEXPmaps <- function(z, Q, pid, N) {
  e <- eigen(Q)
  lefts <- e$vectors
  rights <- solve(lefts)
  d <- diag(e$values)
  .Call('phylomap_hip_exp_maps', PACKAGE = 'phylomap', z, Q, as.numeric(pid), as.integer(N), lefts, rights, d,
        isTRUE(getOption("phylomap.hip.rescale", FALSE)))
}

# The tree z carrying history r (1-based) of h (a simulate_maps() or sumstatEXPmaps() result, or its $maps): named maps
# (names = states, as phytools stores them), mapnames, node.states (E x 2), mapped.edge (E x n, columns named by state) and
# the history's tip states -- divtophy's result, accepted as the input tree of sumstatMCMC / SPARSEsumstatMCMC / sumstatEXP.
history_tree <- function(z, h, r, n = NULL) {
  m <- if (!is.null(h$maps)) h$maps else h
  E <- m$n_edge
  stopifnot(nrow(z$edge) == E, r >= 1, r <= m$n_hist)
  rows <- (r - 1) * E + seq_len(E)
  lo <- m$off[rows] + 1
  hi <- m$off[rows + 1]
  if (is.null(n)) n <- max(m$state[lo[1]:hi[E]])
  z$maps <- vector("list", E)
  z$mapnames <- vector("list", E)
  z$node.states <- matrix(0L, nrow = E, ncol = 2)
  z$mapped.edge <- matrix(0, nrow = E, ncol = n, dimnames = list(NULL, as.character(seq_len(n))))
  for (b in seq_len(E)) {
    s <- m$state[lo[b]:hi[b]]
    d <- m$dwell[lo[b]:hi[b]]
    names(d) <- s
    z$maps[[b]] <- d
    z$mapnames[[b]] <- as.integer(s)
    z$node.states[b, ] <- c(s[1], s[length(s)])
    for (i in seq_along(s)) z$mapped.edge[b, s[i]] <- z$mapped.edge[b, s[i]] + d[i]
  }
  ntips <- length(z$states)
  tip_rows <- which(z$edge[, 2] <= ntips)
  z$states[z$edge[tip_rows, 2]] <- z$node.states[tip_rows, 2]
  z
}
