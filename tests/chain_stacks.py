"""Small ``nn.Sequential`` stacks that reach the between-stage decisions of ``ali_hip.chain`` no shipped model does:
name -> (constructor, NHWC input shape [B,H,W,Cp], logical input channels).  tests/test_chain_routes.py pins their
routes on the meta device, tests/test_gpu_chain_stacks.py runs them (and the ``SYNTHETIC`` stacks of
test_chain_routes.py) against fp64 autograd on the device.  The comment of a stack names the decision it is there for."""
import torch.nn as nn

NEW_STACKS = {
    # fold_ok is False behind a Tanh: the mask goes through rowmask_mul, act_bwd runs for the Tanh
    "tanh_drop": (lambda: nn.Sequential(nn.Conv2d(4, 16, 3), nn.Tanh(), nn.Dropout2d(0.3), nn.Conv2d(16, 8, (3, 2)),
                                        nn.LeakyReLU(0.2)), (3, 7, 6, 4), 4),
    # bn_leave is False behind a ConvT: ali_bn_stats on its own, bn_apply with mask_post; backward epilogue on the
    # convT data-gradient route
    "convT_bn_drop": (lambda: nn.Sequential(nn.ConvTranspose2d(16, 8, 4, stride=2), nn.LeakyReLU(0.2), nn.BatchNorm2d(8),
                                            nn.Dropout2d(0.25), nn.ConvTranspose2d(8, 4, 3), nn.Tanh()), (3, 3, 4, 16), 16),
    # stand-alone statistics through mask_in; the backward reductions ride a conv data gradient
    "convT_drop_bn": (lambda: nn.Sequential(nn.ConvTranspose2d(16, 8, 4, stride=2), nn.LeakyReLU(0.2), nn.Dropout2d(0.25),
                                            nn.BatchNorm2d(8), nn.Conv2d(8, 12, 3), nn.LeakyReLU(0.2)), (3, 3, 4, 16), 16),
    # BatchNorm in front of a Flatten + Linear: the conv leaves partials for a "flat" stage
    "bn_flat": (lambda: nn.Sequential(nn.Conv2d(3, 8, 3), nn.LeakyReLU(0.2), nn.BatchNorm2d(8), nn.Flatten(),
                                      nn.Linear(96, 5)), (5, 6, 5, 4), 3),
    # ReLU as slope 0, forward and derivative
    "relu": (lambda: nn.Sequential(nn.Conv2d(4, 12, 3), nn.ReLU(), nn.Conv2d(12, 8, 3, stride=2), nn.ReLU(),
                                   nn.Conv2d(8, 4, 1)), (3, 9, 8, 4), 4),
    # a scatter_gemm stage that must fold the next stage's mask (runs the GEMM of its kind); a 2-channel map
    "scatter_drop": (lambda: nn.Sequential(nn.ConvTranspose2d(32, 2, 5, stride=2), nn.LeakyReLU(0.2), nn.Dropout2d(0.25),
                                           nn.Conv2d(2, 8, 3), nn.LeakyReLU(0.2)), (3, 4, 5, 32), 32),
    # a head stage with ["bn", "drop"] in front of it, on a 1x1 map
    "head_after_bn_drop": (lambda: nn.Sequential(nn.Conv2d(8, 16, 1), nn.LeakyReLU(0.1), nn.BatchNorm2d(16),
                                                 nn.Dropout2d(0.2), nn.Conv2d(16, 1, 1)), (6, 1, 1, 8), 8),
    # batch statistics in eval mode too, no running buffers
    "bn_norun": (lambda: nn.Sequential(nn.Conv2d(4, 8, 3), nn.LeakyReLU(0.2),
                                       nn.BatchNorm2d(8, track_running_stats=False), nn.Conv2d(8, 4, 2)), (3, 6, 5, 4), 4),
    # linear_repack / unflat on a padded input (10 of 12 channels), stand-alone BatchNorm into a ConvT
    "linear_unflat_bn": (lambda: nn.Sequential(nn.Linear(10, 48), nn.Unflatten(1, (12, 2, 2)), nn.LeakyReLU(0.2),
                                               nn.BatchNorm2d(12), nn.ConvTranspose2d(12, 4, 3, stride=2)),
                         (4, 1, 1, 12), 10),
    # one-channel ends the direct kernels refuse (128 channels: 25 / 16 taps need 13 / 8 accumulators per thread, the
    # weight-gradient kernel has 7): the first conv's weight gradient and the whole tail take the GEMMs of their kind.
    # (New names go last in sorted order: test_gpu_chain_stacks.build seeds a stack by its sorted position.)
    "wide_first_k5": (lambda: nn.Sequential(nn.Conv2d(3, 128, 5), nn.LeakyReLU(0.2)), (4, 7, 8, 4), 3),
    "wide_tail_k4": (lambda: nn.Sequential(nn.ConvTranspose2d(128, 1, 4), nn.Tanh()), (4, 5, 6, 128), 128),
}
