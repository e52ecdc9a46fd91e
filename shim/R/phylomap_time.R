# Exact state probabilities and expected statistics through time on the GPU (shim/phylomap_time_shim.cpp ->
# phm_expected_through_time): when on the tree the dwell and the jumps fall, with no sampling.  Drop this file into the package's R/
# directory.
#
# Depth runs from the root: 0 there, a child's depth its parent's plus the edge length (an age is the largest tip depth minus a
# depth, on an ultrametric tree).
# sumstatExpectedTime(tree, Q, pid, bounds): list(loglik = log p(tips | Q) per site;
#   occupancy = S x K x n, the expected number of lineages in each state at each depth in bounds (a node at a bound counts through
#   its parent branch; a bound of 0 counts the root);
#   bins = S x (K - 1) x (n + n(n-1)) when K >= 2, E[dwell_i] and E[N_ij] within [bounds[k], bounds[k + 1]) in the column order of
#   sumstatMCMC (man/sumstatMCMC.Rd);
#   points = S x P x n, P(state at the point | tips), when points is a P x 2 matrix of (1-based edge row, distance from the
#   parent end)).
# sites: NULL (one site, tree$states) or an S x n_tips matrix of tip states (0 = missing).  observe: as for sumstatExpected.
sumstatExpectedTime <- function(tree, Q, pid, bounds, points = NULL, sites = NULL, observe = NULL) {
  if (is.null(sites)) sites <- matrix(as.integer(round(tree$states)), nrow = 1)
  storage.mode(sites) <- "integer"
  obs <- if (is.null(observe)) integer(0) else as.integer(observe)
  pts <- if (is.null(points)) matrix(0, 0, 2) else matrix(as.numeric(points), ncol = 2)
  b <- if (is.null(bounds)) numeric(0) else as.numeric(bounds)
  out <- .Call('phylomap_expected_through_time', PACKAGE = 'phylomap', tree, sites, Q, as.numeric(pid), obs, b, pts)
  S <- nrow(sites)
  n <- nrow(Q)
  K <- length(b)
  if (!is.null(out$occupancy)) dim(out$occupancy) <- c(S, K, n)
  if (!is.null(out$bins)) dim(out$bins) <- c(S, K - 1, n * n)
  if (!is.null(out$points)) dim(out$points) <- c(S, nrow(pts), n)
  out
}
