# Forward simulation of character histories on the GPU (shim/phylomap_simulate_shim.cpp -> phm_simulate_histories): the device
# replacement of sample2statehistory / samplethebranch (R/sourceme.R:346-414) and of simulate_2_state_tree /
# simulate_4_state_tree (R/simulate_*_state_tree.R), R histories per call.  set.seed() controls the result.  Drop this file into
# the package's R/ directory; the wrappers of the same name replace the interpreted ones.

# R independent histories: list(tips = R x n_tips (1-based, reported through `observe`), stats = R x (n + n*n + 1): dwell per state,
# jump counts n x n row-major (from, to), root state (0-based); nodes = R x (n_tips + Nnode) true states when nodes = TRUE).
# observe: NULL (identity) or n values in 1..n, e.g. c(1, 2, 1, 2) for simulate_4_state_tree's parity map.
# The tips matrix is what the samplers take as z$sites (shim/R/phylomap_hip_options.R, sumstat_sites).
simulate_histories <- function(tree, Q, pid, R = 1, observe = NULL, nodes = FALSE) {
  obs <- if (is.null(observe)) integer(0) else as.integer(observe)
  .Call('phylomap_hip_simulate_histories', PACKAGE = 'phylomap', tree, Q, as.numeric(pid), as.integer(R), obs, isTRUE(nodes))
}

# sample2statehistory(tree, Q, pid) for two states: c(nodestates, n01, n10, t0, t1), node states by ape node id (1-based).
# n01 / n10 are the 1 -> 2 / 2 -> 1 jumps (countgains / countlosses); for n > 2 the reference counts only +-1 steps
# (R/sourceme.R:343-344): use simulate_histories() for the full jump matrix.
sample2statehistory <- function(tree, Q, pid) {
  stopifnot(nrow(Q) == 2)
  h <- simulate_histories(tree, Q, pid, R = 1, nodes = TRUE)
  s <- h$stats[1, ]
  c(h$nodes[1, ], s[4], s[5], s[1], s[2])        # stats: t0, t1, n00, n01, n10, n11, root
}

# simulate_2_state_tree / simulate_4_state_tree for any tree and model: the tree with simulated tip states, every tip branch
# re-initialised to two half-length pieces (1, tip state), node.states 1 except the tips (R/simulate_2_state_tree.R:15-31).
# observe = c(1, 2, 1, 2) is simulate_4_state_tree; `seed`, when given, is passed to set.seed() as the reference does.
simulate_state_tree <- function(seed = NULL, atree, Q, pid, observe = NULL) {
  if (!is.null(seed)) set.seed(seed)
  tipstates <- simulate_histories(atree, Q, pid, R = 1, observe = observe)$tips[1, ]
  ntips <- length(tipstates)
  atree$states <- tipstates
  atree$node.states <- matrix(1L, nrow = nrow(atree$edge), ncol = 2)
  for (row in which(atree$edge[, 2] <= ntips)) {
    j <- atree$edge[row, 2]
    atree$maps[[row]] <- rep(atree$edge.length[row] / 2, 2)
    names(atree$maps[[row]]) <- c(1, tipstates[j])
    atree$node.states[row, 2] <- tipstates[j]
  }
  atree$mapnames <- lapply(atree$maps, function(m) as.integer(names(m)))
  atree
}
