"""bayesianfiltering_amd: MI355X-native batched Bayesian filtering (Kalman / Gaussian-sum /
bootstrap particle filters) behind the call surface of the reference package ``gaussfiltax``
(kostastsa/BayesianFiltering).  See DESIGN.md for the hot path and its boundary."""
from .models import ParamsNLSSM, ParamsBPF, NonlinearSSM
from .containers import GaussianComponent, GaussianSum
from .inference import (PosteriorGaussianSumFiltered, gaussian_sum_filter, unscented_gaussian_sum_filter, ParamsUKF,
                        speedy_augmented_gaussian_sum_filter, augmented_gaussian_sum_filter,
                        speedy_unscented_agsf, unscented_agsf, augmented_gaussian_sum_filter_optimal, optimal_resampling,
                        kalman_filter, FilterCarry,
                        FULL5, FILTERED, PRNGKey, sample_initial_component_means,
                        bootstrap_particle_filter, ParticleCarry, resample_indices)
from .smoother import (PosteriorGaussianSmoothed, SmootherCarry, rts_smoother, kalman_smoother,
                       extended_kalman_smoother, unscented_kalman_smoother)
from .gaussian_sum_smoother import (PosteriorGaussianSumSmoothed, GaussianSumSmootherCarry, gaussian_sum_smoother,
                                    extended_gaussian_sum_smoother, unscented_gaussian_sum_smoother)
from .gaussian_sum_sampler import (GaussianSumSamplerCarry, gaussian_sum_posterior_sample,
                                   extended_gaussian_sum_posterior_sample, unscented_gaussian_sum_posterior_sample)
from .sampler import (SamplerCarry, posterior_sample, kalman_posterior_sample, extended_kalman_posterior_sample,
                      unscented_kalman_posterior_sample)
from .particle_sampler import (ParticleSamplerCarry, particle_posterior_sample, bootstrap_particle_posterior_sample)
from .parallel import (parallel_kalman_filter, parallel_kalman_workspace_bytes, parallel_rts_smoother,
                       parallel_rts_workspace_bytes, parallel_kalman_smoother, parallel_posterior_sample,
                       parallel_ffbs_workspace_bytes, parallel_kalman_posterior_sample)
from ._lib import BayesFiltError
from . import nonlinearities, utils

__all__ = ["ParamsNLSSM", "ParamsBPF", "NonlinearSSM", "GaussianComponent", "GaussianSum", "PosteriorGaussianSumFiltered",
           "gaussian_sum_filter", "unscented_gaussian_sum_filter", "ParamsUKF", "speedy_augmented_gaussian_sum_filter", "augmented_gaussian_sum_filter", "speedy_unscented_agsf", "unscented_agsf", "augmented_gaussian_sum_filter_optimal", "optimal_resampling", "kalman_filter", "FilterCarry", "FULL5", "FILTERED", "PRNGKey",
           "sample_initial_component_means", "bootstrap_particle_filter", "ParticleCarry", "resample_indices",
           "nonlinearities", "utils", "BayesFiltError",
           "PosteriorGaussianSmoothed", "SmootherCarry", "rts_smoother", "kalman_smoother", "extended_kalman_smoother", "unscented_kalman_smoother",
           "PosteriorGaussianSumSmoothed", "GaussianSumSmootherCarry", "gaussian_sum_smoother", "extended_gaussian_sum_smoother",
           "unscented_gaussian_sum_smoother", "GaussianSumSamplerCarry", "gaussian_sum_posterior_sample",
           "extended_gaussian_sum_posterior_sample", "unscented_gaussian_sum_posterior_sample",
           "SamplerCarry", "posterior_sample", "kalman_posterior_sample", "extended_kalman_posterior_sample", "unscented_kalman_posterior_sample",
           "ParticleSamplerCarry", "particle_posterior_sample", "bootstrap_particle_posterior_sample",
           "parallel_kalman_filter", "parallel_kalman_workspace_bytes", "parallel_rts_smoother", "parallel_rts_workspace_bytes",
           "parallel_kalman_smoother", "parallel_posterior_sample", "parallel_ffbs_workspace_bytes",
           "parallel_kalman_posterior_sample"]
