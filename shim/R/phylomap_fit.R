# Log-likelihood of many rate matrices in one GPU call (shim/phylomap_loglik_shim.cpp -> phm_loglik_models) and the
# maximum-likelihood fit on top of it.  Drop this file into the package's R/ directory.

# sumstatLoglik(tree, Qs, pid): log p(tips | Q_k) for K rate matrices.  Qs: an n x n matrix, an n x n x K array or a list of
# n x n matrices.  pid: n values shared by every model, or an n x K matrix.  sites: NULL (one site, tree$states) or an
# S x n_tips matrix of tip states (0 = missing).  observe: NULL (identity) or n values in 1..n, e.g. c(1, 2, 1, 2) for the
# parity tips of sumstatMCMCks.  site_of_model: NULL -- every model on every site, an S x K matrix is returned -- or K site
# indices (1-based): model k on its own site alone, K values are returned.  An impossible evaluation is -Inf.
sumstatLoglik <- function(tree, Qs, pid, sites = NULL, observe = NULL, site_of_model = NULL) {
  if (is.list(Qs)) Qs <- array(unlist(Qs), dim = c(nrow(Qs[[1]]), ncol(Qs[[1]]), length(Qs)))
  if (is.matrix(Qs)) Qs <- array(Qs, dim = c(dim(Qs), 1))
  n <- dim(Qs)[1]
  if (is.null(sites)) sites <- matrix(as.integer(round(tree$states)), nrow = 1)
  storage.mode(sites) <- "integer"
  obs <- if (is.null(observe)) integer(0) else as.integer(observe)
  som <- if (is.null(site_of_model)) integer(0) else as.integer(site_of_model)
  out <- .Call('phylomap_loglik_models', PACKAGE = 'phylomap', tree, sites, as.numeric(Qs), as.integer(n), as.numeric(pid), obs, som)
  if (is.null(site_of_model)) dim(out) <- c(nrow(sites), dim(Qs)[3])
  out
}

# The fit itself is left to R's own optimiser: the Python layer's lock-step BFGS (phylomap_amd/fit.py) is not restated here.
# For a model theta -> Q (make_Q) fitted jointly over the sites, in log theta:
#
#   nll <- function(x) -sum(sumstatLoglik(tree, make_Q(exp(x)), pid, sites))
#   fit <- optim(log(theta0), nll, method = "BFGS", control = list(reltol = 1e-12))
#   theta_hat <- exp(fit$par); aic <- 2 * length(theta_hat) + 2 * fit$value
#
# optim evaluates one model per call; to use the batch, hand it a gradient that evaluates its 2p central-difference points in
# one call:
#
#   gr <- function(x, h = 1e-4) {
#     p <- length(x)
#     pts <- rbind(diag(h, p), -diag(h, p)) + matrix(x, 2 * p, p, byrow = TRUE)
#     ll <- colSums(sumstatLoglik(tree, lapply(seq_len(2 * p), function(k) make_Q(exp(pts[k, ]))), pid, sites))
#     -(ll[1:p] - ll[p + 1:p]) / (2 * h)
#   }
#   fit <- optim(log(theta0), nll, gr, method = "BFGS")
