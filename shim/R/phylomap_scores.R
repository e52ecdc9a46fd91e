# Expected statistics of many rate matrices in one GPU call (shim/phylomap_scores_shim.cpp -> phm_expected_stats_models): what an
# exact score, an observed information matrix or an EM step needs at many Q.  Drop this file into the package's R/ directory.

# sumstatExpectedModels(tree, Qs, pid): E[dwell_i | tips, Q_k] and E[N_ij | tips, Q_k], summed over the tree, with
# log p(tips | Q_k), for K rate matrices.  The arguments are sumstatLoglik's (phylomap_fit.R).  Returns list(stats, loglik).
# site_of_model NULL: stats is S x K x (n + n(n-1)) and loglik S x K.  With K site indices (1-based): stats is
# K x (n + n(n-1)) and loglik has K values.  The columns are sumstatMCMC's: n dwell times, then the counts row by row without the
# diagonal.  An impossible evaluation is -Inf with NaN statistics.
sumstatExpectedModels <- function(tree, Qs, pid, sites = NULL, observe = NULL, site_of_model = NULL) {
  if (is.list(Qs)) Qs <- array(unlist(Qs), dim = c(nrow(Qs[[1]]), ncol(Qs[[1]]), length(Qs)))
  if (is.matrix(Qs)) Qs <- array(Qs, dim = c(dim(Qs), 1))
  n <- dim(Qs)[1]
  K <- dim(Qs)[3]
  if (is.null(sites)) sites <- matrix(as.integer(round(tree$states)), nrow = 1)
  storage.mode(sites) <- "integer"
  obs <- if (is.null(observe)) integer(0) else as.integer(observe)
  som <- if (is.null(site_of_model)) integer(0) else as.integer(site_of_model)
  out <- .Call('phylomap_expected_stats_models', PACKAGE = 'phylomap', tree, sites, as.numeric(Qs), as.integer(n), as.numeric(pid), obs, som)
  if (is.null(site_of_model)) {
    dim(out$stats) <- c(nrow(sites), K, n * n)
    dim(out$loglik) <- c(nrow(sites), K)
  } else {
    dim(out$stats) <- c(K, n * n)
  }
  out
}

# The exact score of a model theta -> Q (make_Q) in log theta, for an index model whose entry (i, j) is parameter idx[i, j]
# (0 = structurally zero), from one row `s` of stats:
#
#   score <- function(theta, s, idx) sapply(seq_along(theta), function(c) {
#     ij <- which(idx == c, arr.ind = TRUE); n <- nrow(idx)
#     col <- n + (ij[, 1] - 1) * (n - 1) + ifelse(ij[, 2] < ij[, 1], ij[, 2], ij[, 2] - 1)
#     sum(s[col] - theta[c] * s[ij[, 1]])
#   })
