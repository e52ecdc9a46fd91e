# Exact conditional expectations on the GPU (shim/phylomap_expected_shim.cpp -> phm_expected_stats): E[dwell_i | tips, Q] and
# E[N_ij | tips, Q] with no sampling (Minin & Suchard 2008), the numbers the posterior means of sumstatMCMC & co. converge to.
# Drop this file into the package's R/ directory.

# sumstatExpected(tree, Q, pid): list(stats = S x (n + n(n-1)) in the column order of sumstatMCMC (man/sumstatMCMC.Rd),
# loglik = log p(tips | Q) per site; branch = S x n_edge x (n + n(n-1)) by edge row when per_branch = TRUE; nodes =
# S x (n_tips + Nnode) x n, P(state of node | tips) by ape node id, when nodes = TRUE).
# sites: NULL (one site, tree$states) or an S x n_tips matrix of tip states (0 = missing), e.g. simulate_histories()$tips.
# observe: NULL (identity) or n values in 1..n, e.g. c(1, 2, 1, 2) for the parity tips of sumstatMCMCks.
sumstatExpected <- function(tree, Q, pid, sites = NULL, observe = NULL, per_branch = FALSE, nodes = FALSE) {
  if (is.null(sites)) sites <- matrix(as.integer(round(tree$states)), nrow = 1)
  storage.mode(sites) <- "integer"
  obs <- if (is.null(observe)) integer(0) else as.integer(observe)
  out <- .Call('phylomap_expected_stats', PACKAGE = 'phylomap', tree, sites, Q, as.numeric(pid), obs, isTRUE(per_branch), isTRUE(nodes))
  n <- nrow(Q)
  if (!is.null(out$branch)) dim(out$branch) <- c(nrow(sites), nrow(tree$edge), n * n)
  if (!is.null(out$nodes)) dim(out$nodes) <- c(nrow(sites), ncol(sites) + tree$Nnode, n)
  out
}
