"""Which kernels serve which stage (ali_hip.chain.route), pinned for every stage of the five chains (E.layers, G.layers,
D.dx, D.dz, D.dxz) of the four benchmark configurations -- at the batch sizes, image sizes and channel strides the
stepper feeds them in ``bench.py`` -- and for synthetic stacks that reach the routes no benchmark model does.

No GPU and no forward pass: the models are built on the meta device, the library's host-side queries
(``ali_tconv_scatter_ok``) run on the CPU.  The expected tables were recorded by evaluating the predicates of the
commit before ``route`` existed (``_is_tconv1``, ``_is_head``, ``_scatter_fwd``, ``_scatter_dgrad``, ``_first_conv_direct``
and the ``if`` ladders of the two generators) -- not by running ``route``.

A row is (kind, pre-op pattern, fwd, wgrad, wgrad_fold, dgrad, planes, fold_ok, bn_leave, bn_reduce): the stage's kind
and the fields of its ``Route`` (``planes``: the form a single requested plane takes).  The second list of a chain is
``wgrad_geoms``: the (B,H,W,C,P,Q,K,R,S,stride,pad) that size the split of every deferred weight gradient -- the
summation order, hence the bits, of the weight gradients depend on it.

This file only names routes.  The synthetic stacks -- ``SYNTHETIC`` here and ``chain_stacks.NEW_STACKS``, whose rows and
stage shapes ``NEW_EXPECTED`` pins -- are RUN in tests/test_gpu_chain_stacks.py: ``run_chain`` on the device against
fp64 autograd, forward, input gradient, parameter gradients and BatchNorm buffers."""
import importlib

import pytest
import torch
import torch.nn as nn

MODULES = {"mnist": "image_scms.mnist", "audio": "image_scms.audio_mnist", "whale": "image_scms.whalecalls",
           "esrf": "image_scms.esrf_acoustic"}
CONV = ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True)
CONVT = ('convT', [], 'convT', ('convT', 'colsum'), ('convT', 'colsum'), 'convT', None, True, False, True)

# configuration -> chain -> (input shape [B,H,W,Cp], logical input channels, rows, wgrad_geoms)
BENCH_EXPECTED = {
    "mnist": {
        "E": ((512, 28, 28, 8), 5, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (512, 28, 28, 8, 14, 14, 64, 3, 3, 2, 1),
            (512, 14, 14, 64, 7, 7, 128, 4, 4, 2, 1),
            (512, 7, 7, 128, 3, 3, 256, 4, 4, 2, 1),
            (512, 3, 3, 256, 1, 1, 512, 4, 4, 2, 1),
            (512, 1, 1, 512, 1, 1, 512, 1, 1, 2, 0),
        ]),
        "G": ((512, 1, 1, 800), 771, [
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            ('convT', [], 'tconv1', ('tconv1', 'colsum'), ('tconv1', 'colsum'), 'tconv1', None, False, False, False),
        ], [
            (512, 3, 3, 512, 1, 1, 800, 3, 3, 1, 0),
            (512, 7, 7, 256, 3, 3, 512, 3, 3, 2, 0),
            (512, 13, 13, 128, 7, 7, 256, 3, 3, 2, 1),
            (512, 25, 25, 64, 13, 13, 128, 3, 3, 2, 1),
        ]),
        "dx": ((512, 28, 28, 8), 5, [
            ('conv', ['drop'], 'conv', ('first_direct', 'colsum'), ('conv', 'fused'), 'conv', 'direct', True, True, True),
            ('conv', ['drop', 'bn'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
            ('conv', ['bn', 'drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
            ('conv', ['bn', 'drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
            ('conv', ['bn', 'drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
        ], [
            (512, 28, 28, 8, 24, 24, 32, 5, 5, 1, 0),
            (512, 24, 24, 32, 11, 11, 64, 4, 4, 2, 0),
            (512, 11, 11, 64, 8, 8, 128, 4, 4, 1, 0),
            (512, 8, 8, 128, 3, 3, 256, 4, 4, 2, 0),
            (512, 3, 3, 256, 1, 1, 512, 3, 3, 1, 0),
        ]),
        "dz": ((512, 1, 1, 512), 512, [
            ('conv', ['drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            ('conv', ['drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
        ], [
            (512, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
            (512, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
        ]),
        "dxz": ((512, 1, 1, 1024), 1024, [
            ('conv', ['drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            ('conv', ['drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
            ('conv', ['drop'], 'head', ('head', 'fused'), ('head', 'fused'), 'conv', None, True, True, True),
        ], [
            (512, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (512, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (512, 1, 1, 1024, 1, 1, 1, 1, 1, 1, 0),
        ]),
    },
    "audio": {
        "E": ((256, 128, 128, 8), 7, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (256, 128, 128, 8, 63, 63, 64, 5, 5, 2, 1),
            (256, 63, 63, 64, 31, 31, 128, 5, 5, 2, 1),
            (256, 31, 31, 128, 15, 15, 256, 5, 5, 2, 1),
            (256, 15, 15, 256, 7, 7, 512, 5, 5, 2, 1),
            (256, 7, 7, 512, 3, 3, 1024, 5, 5, 2, 1),
            (256, 3, 3, 1024, 1, 1, 512, 5, 5, 2, 1),
        ]),
        "G": ((256, 1, 1, 2048), 2048, [
            ('linear', [], 'conv', ('linear_repack', 'unflat'), ('linear_repack', 'unflat'), 'conv', None, False, False, False),
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            ('convT', [], 'scatter', ('convT_scatter', 'colsum'), ('convT_scatter', 'colsum'), 'convT', None, False, False, True),
        ], [
            (256, 1, 1, 2048, 1, 1, 16384, 1, 1, 1, 0),
            (256, 8, 8, 512, 4, 4, 1024, 5, 5, 2, 2),
            (256, 16, 16, 256, 8, 8, 512, 5, 5, 2, 2),
            (256, 32, 32, 128, 16, 16, 256, 5, 5, 2, 2),
            (256, 64, 64, 64, 32, 32, 128, 5, 5, 2, 2),
            (256, 128, 128, 1, 64, 64, 64, 5, 5, 2, 2),
        ]),
        "dx": ((256, 128, 128, 8), 7, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (256, 128, 128, 8, 63, 63, 64, 5, 5, 2, 1),
            (256, 63, 63, 64, 31, 31, 128, 5, 5, 2, 1),
            (256, 31, 31, 128, 15, 15, 256, 5, 5, 2, 1),
            (256, 15, 15, 256, 7, 7, 512, 5, 5, 2, 1),
            (256, 7, 7, 512, 3, 3, 1024, 5, 5, 2, 1),
            (256, 3, 3, 1024, 1, 1, 512, 5, 5, 2, 1),
        ]),
        "dz": ((256, 1, 1, 512), 512, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
        ], [
            (256, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
            (256, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
        ]),
        "dxz": ((256, 1, 1, 1024), 1024, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            ('conv', [], 'head', ('head', 'fused'), ('head', 'fused'), 'conv', None, True, True, True),
        ], [
            (256, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (256, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (256, 1, 1, 1024, 1, 1, 1, 1, 1, 1, 0),
        ]),
    },
    "whale": {
        "E": ((128, 256, 256, 4), 2, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (128, 256, 256, 4, 127, 127, 64, 5, 5, 2, 1),
            (128, 127, 127, 64, 63, 63, 128, 5, 5, 2, 1),
            (128, 63, 63, 128, 31, 31, 256, 5, 5, 2, 1),
            (128, 31, 31, 256, 15, 15, 512, 5, 5, 2, 1),
            (128, 15, 15, 512, 7, 7, 1024, 5, 5, 2, 1),
            (128, 7, 7, 1024, 3, 3, 1024, 5, 5, 2, 1),
            (128, 3, 3, 1024, 1, 1, 512, 5, 5, 2, 1),
        ]),
        "G": ((128, 1, 1, 768), 768, [
            ('linear', [], 'conv', ('linear_repack', 'unflat'), ('linear_repack', 'unflat'), 'conv', None, False, False, False),
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            ('convT', [], 'scatter', ('convT_scatter', 'colsum'), ('convT_scatter', 'colsum'), 'convT', None, False, False, True),
        ], [
            (128, 1, 1, 768, 1, 1, 16384, 1, 1, 1, 0),
            (128, 8, 8, 1024, 4, 4, 1024, 5, 5, 2, 2),
            (128, 16, 16, 512, 8, 8, 1024, 5, 5, 2, 2),
            (128, 32, 32, 256, 16, 16, 512, 5, 5, 2, 2),
            (128, 64, 64, 128, 32, 32, 256, 5, 5, 2, 2),
            (128, 128, 128, 64, 64, 64, 128, 5, 5, 2, 2),
            (128, 256, 256, 1, 128, 128, 64, 5, 5, 2, 2),
        ]),
        "dx": ((128, 256, 256, 4), 2, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (128, 256, 256, 4, 127, 127, 64, 5, 5, 2, 1),
            (128, 127, 127, 64, 63, 63, 128, 5, 5, 2, 1),
            (128, 63, 63, 128, 31, 31, 128, 5, 5, 2, 1),
            (128, 31, 31, 128, 15, 15, 256, 5, 5, 2, 1),
            (128, 15, 15, 256, 7, 7, 512, 5, 5, 2, 1),
            (128, 7, 7, 512, 3, 3, 1024, 5, 5, 2, 1),
            (128, 3, 3, 1024, 1, 1, 512, 5, 5, 2, 1),
        ]),
        "dz": ((128, 1, 1, 512), 512, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
        ], [
            (128, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
            (128, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
        ]),
        "dxz": ((128, 1, 1, 1024), 1024, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            ('conv', [], 'head', ('head', 'fused'), ('head', 'fused'), 'conv', None, True, True, True),
        ], [
            (128, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (128, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (128, 1, 1, 1024, 1, 1, 1, 1, 1, 1, 0),
        ]),
    },
    "esrf": {
        "E": ((64, 512, 512, 4), 3, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (64, 512, 512, 4, 255, 255, 64, 5, 5, 2, 1),
            (64, 255, 255, 64, 127, 127, 128, 5, 5, 2, 1),
            (64, 127, 127, 128, 63, 63, 256, 5, 5, 2, 1),
            (64, 63, 63, 256, 31, 31, 512, 5, 5, 2, 1),
            (64, 31, 31, 512, 15, 15, 1024, 5, 5, 2, 1),
            (64, 15, 15, 1024, 7, 7, 2048, 5, 5, 2, 1),
            (64, 7, 7, 2048, 3, 3, 4096, 5, 5, 2, 1),
            (64, 3, 3, 4096, 1, 1, 512, 5, 5, 2, 1),
        ]),
        "G": ((64, 1, 1, 800), 769, [
            ('linear', [], 'conv', ('linear_repack', 'unflat'), ('linear_repack', 'unflat'), 'conv', None, False, False, False),
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            CONVT,
            ('convT', [], 'scatter', ('convT_scatter', 'colsum'), ('convT_scatter', 'colsum'), 'convT', None, False, False, True),
        ], [
            (64, 1, 1, 800, 1, 1, 16384, 1, 1, 1, 0),
            (64, 8, 8, 1024, 4, 4, 1024, 5, 5, 2, 2),
            (64, 16, 16, 512, 8, 8, 1024, 5, 5, 2, 2),
            (64, 32, 32, 256, 16, 16, 512, 5, 5, 2, 2),
            (64, 64, 64, 128, 32, 32, 256, 5, 5, 2, 2),
            (64, 128, 128, 64, 64, 64, 128, 5, 5, 2, 2),
            (64, 256, 256, 64, 128, 128, 64, 5, 5, 2, 2),
            (64, 512, 512, 1, 256, 256, 64, 5, 5, 2, 2),
        ]),
        "dx": ((64, 512, 512, 4), 3, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
            CONV,
        ], [
            (64, 512, 512, 4, 255, 255, 64, 5, 5, 2, 1),
            (64, 255, 255, 64, 127, 127, 128, 5, 5, 2, 1),
            (64, 127, 127, 128, 63, 63, 256, 5, 5, 2, 1),
            (64, 63, 63, 256, 31, 31, 512, 5, 5, 2, 1),
            (64, 31, 31, 512, 15, 15, 1024, 5, 5, 2, 1),
            (64, 15, 15, 1024, 7, 7, 2048, 5, 5, 2, 1),
            (64, 7, 7, 2048, 3, 3, 4096, 5, 5, 2, 1),
            (64, 3, 3, 4096, 1, 1, 512, 5, 5, 2, 1),
        ]),
        "dz": ((64, 1, 1, 512), 512, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
        ], [
            (64, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
            (64, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
        ]),
        "dxz": ((64, 1, 1, 1024), 1024, [
            ('conv', [], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', 'scatter', True, True, True),
            CONV,
            ('conv', [], 'head', ('head', 'fused'), ('head', 'fused'), 'conv', None, True, True, True),
        ], [
            (64, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (64, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
            (64, 1, 1, 1024, 1, 1, 1, 1, 1, 1, 0),
        ]),
    },
}

SYNTHETIC = {
    # GEMM + col2im scatter fallback (two channels out of 32: the one-launch kernel refuses), then a stride-1 one-channel
    # tail that the direct kernels take at a channel stride of 64 ...
    "scatter_gemm": (lambda: nn.Sequential(nn.ConvTranspose2d(32, 2, 5, stride=2), nn.LeakyReLU(0.2)), (4, 8, 8, 32), 32),
    "tconv1_tanh": (lambda: nn.Sequential(nn.ConvTranspose2d(64, 1, 3), nn.Tanh()), (4, 8, 8, 64), 64),
    # ... and not at 48 (scatter form, one channel; too wide for the one-launch kernel's LDS tile)
    "tail_48": (lambda: nn.Sequential(nn.ConvTranspose2d(48, 1, 3), nn.Tanh()), (4, 8, 8, 48), 48),
    # plain Linear layers (with and without bias), Linear + Unflatten onto a 1x1 map
    "linear": (lambda: nn.Sequential(nn.Linear(16, 32), nn.LeakyReLU(0.2), nn.Linear(32, 8, bias=False), nn.Tanh(),
                                     nn.Linear(8, 12), nn.Unflatten(1, (12, 1, 1))), (4, 1, 1, 16), 16),
    # a direct first conv on an unpadded 3-channel input (no GEMM job for the combined launch), Tanh (no mask fold),
    # a 1-channel 1x1 conv on a 6x6 map (not the head GEMV) behind BatchNorm
    "first_unpadded": (lambda: nn.Sequential(nn.Conv2d(3, 32, 3), nn.Tanh(), nn.BatchNorm2d(32), nn.Conv2d(32, 1, 1)),
                       (4, 8, 8, 3), 3),
    # first convs without a plane form: BatchNorm in front, output channels not a multiple of 4
    "first_bn": (lambda: nn.Sequential(nn.BatchNorm2d(4), nn.Conv2d(4, 32, 3), nn.LeakyReLU(0.2)), (4, 8, 8, 4), 4),
    "first_k6": (lambda: nn.Sequential(nn.Conv2d(4, 6, 3, stride=2, bias=False)), (4, 9, 9, 4), 4),
    # a head-shaped conv whose input stride is not a multiple of 4; a strided ConvT(64 -> 1) fed 60 real channels
    "head_odd": (lambda: nn.Sequential(nn.Dropout2d(0.2), nn.Conv2d(6, 1, 1)), (4, 1, 1, 6), 6),
    "tail_60": (lambda: nn.Sequential(nn.ConvTranspose2d(60, 1, 5, stride=2, padding=2, output_padding=1)), (4, 8, 8, 64), 60),
}

SYNTHETIC_EXPECTED = {
    "scatter_gemm": ([
        ('convT', [], 'scatter_gemm', ('convT', 'colsum'), ('convT', 'colsum'), 'convT', None, True, False, True),
    ], [
        (4, 19, 19, 2, 8, 8, 32, 5, 5, 2, 0),
    ]),
    "tconv1_tanh": ([
        ('convT', [], 'tconv1', ('tconv1', 'colsum'), ('tconv1', 'colsum'), 'tconv1', None, False, False, False),
    ], [
    ]),
    "tail_48": ([
        ('convT', [], 'scatter_gemm', ('convT', 'colsum'), ('convT', 'colsum'), 'convT', None, False, False, True),
    ], [
        (4, 10, 10, 1, 8, 8, 48, 3, 3, 1, 0),
    ]),
    "linear": ([
        ('linear', [], 'conv', ('linear', 'colsum'), ('linear', 'colsum'), 'conv', None, False, False, False),
        ('linear', [], 'conv', ('linear', None), ('linear', None), 'conv', None, False, False, False),
        ('linear', [], 'conv', ('linear', 'unflat'), ('linear', 'unflat'), 'conv', None, False, False, False),
    ], [
        (4, 1, 1, 16, 1, 1, 32, 1, 1, 1, 0),
        (4, 1, 1, 32, 1, 1, 8, 1, 1, 1, 0),
        (4, 1, 1, 8, 1, 1, 12, 1, 1, 1, 0),
    ]),
    "first_unpadded": ([
        ('conv', [], 'conv', ('first_direct', 'colsum'), ('first_direct', 'colsum'), 'conv', 'direct', False, True, True),
        ('conv', ['bn'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
    ], [
        (4, 8, 8, 3, 6, 6, 32, 3, 3, 1, 0),
        (4, 6, 6, 32, 6, 6, 1, 1, 1, 1, 0),
    ]),
    "first_bn": ([
        ('conv', ['bn'], 'conv', ('first_direct', 'colsum'), ('conv', 'fused'), 'conv', None, True, True, True),
    ], [
        (4, 8, 8, 4, 6, 6, 32, 3, 3, 1, 0),
    ]),
    "first_k6": ([
        ('conv', [], 'conv', ('conv', None), ('conv', None), 'conv', None, True, True, True),
    ], [
        (4, 9, 9, 4, 4, 4, 6, 3, 3, 2, 0),
    ]),
    "head_odd": ([
        ('conv', ['drop'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, True, True),
    ], [
        (4, 1, 1, 6, 1, 1, 1, 1, 1, 1, 0),
    ]),
    "tail_60": ([
        ('convT', [], 'scatter', ('convT', 'colsum'), ('convT', 'colsum'), 'convT', None, True, False, True),
    ], [
        (4, 16, 16, 1, 8, 8, 64, 5, 5, 2, 2),
    ]),
}


def _pre(row, pattern, **fields):
    """``row`` with another pre-op pattern / other Route fields"""
    from ali_hip.chain import Route
    return (row[0], pattern) + tuple(Route(*row[2:])._replace(**fields))


FIRST = _pre(CONV, [], planes='scatter')        # a first Conv2d with 4-aligned output channels and no BatchNorm in front

# chain_stacks.NEW_STACKS: name -> (rows, [input shape, output shape of every stage]); derived by reading ``route``
NEW_EXPECTED = {
    "tanh_drop": ([_pre(FIRST, [], fold_ok=False), _pre(CONV, ['drop'])],
                  [(3, 7, 6, 4), (3, 5, 4, 16), (3, 3, 3, 8)]),
    "convT_bn_drop": ([CONVT, _pre(CONVT, ['bn', 'drop'], fold_ok=False)],
                      [(3, 3, 4, 16), (3, 8, 10, 8), (3, 10, 12, 4)]),
    "convT_drop_bn": ([CONVT, _pre(CONV, ['drop', 'bn'])],
                      [(3, 3, 4, 16), (3, 8, 10, 8), (3, 6, 8, 12)]),
    "bn_flat": ([FIRST, ('flat', ['bn'], 'conv', ('conv', 'fused'), ('conv', 'fused'), 'conv', None, True, False, True)],
                [(5, 6, 5, 4), (5, 4, 3, 8), (5, 1, 1, 5)]),
    "relu": ([FIRST, CONV, CONV],
             [(3, 9, 8, 4), (3, 7, 6, 12), (3, 3, 2, 8), (3, 3, 2, 4)]),
    "scatter_drop": ([('convT', [], 'scatter_gemm', ('convT', 'colsum'), ('convT', 'colsum'), 'convT', None, True, False, True),
                      _pre(CONV, ['drop'])],
                     [(3, 4, 5, 32), (3, 11, 13, 2), (3, 9, 11, 8)]),
    "head_after_bn_drop": ([FIRST, ('conv', ['bn', 'drop'], 'head', ('head', 'fused'), ('head', 'fused'), 'conv', None,
                                    True, True, True)],
                           [(6, 1, 1, 8), (6, 1, 1, 16), (6, 1, 1, 1)]),
    "bn_norun": ([FIRST, _pre(CONV, ['bn'])],
                 [(3, 6, 5, 4), (3, 4, 3, 8), (3, 3, 2, 4)]),
    "linear_unflat_bn": ([('linear', [], 'conv', ('linear_repack', 'unflat'), ('linear_repack', 'unflat'), 'conv', None,
                           False, False, False), _pre(CONVT, ['bn'])],
                         [(4, 1, 1, 12), (4, 2, 2, 12), (4, 5, 5, 4)]),
    # ali_tconv1_wgrad refuses 128 channels x 25 taps: GEMM weight gradient; the plane form (ali_tconv1_fwd) stays direct
    "wide_first_k5": ([_pre(CONV, [], planes='direct')],
                      [(4, 7, 8, 4), (4, 3, 4, 128)]),
    # ... and 128 channels x 16 taps: no "tconv1" on any pass, the tail is the scatter GEMM of `tail_48`
    "wide_tail_k4": ([('convT', [], 'scatter_gemm', ('convT', 'colsum'), ('convT', 'colsum'), 'convT', None, False, False,
                       True)],
                     [(4, 5, 6, 128), (4, 8, 9, 1)]),
}


def _walk(seq, shape, c_log):
    """(rows, wgrad_geoms) of ``seq`` for an input of ``shape`` with ``c_log`` real channels, without running it"""
    from ali_hip import chain
    plan = chain.ChainPlan(seq)
    rows, saved = [], []
    for st in plan.stages:
        sv = chain._Saved()
        sv.in_shape, sv.out_shape = tuple(shape), chain._out_shape(st, *shape)
        sv.geom, sv.route = chain._geom(st, sv.in_shape, sv.out_shape), chain.route(st, sv.in_shape, c_log)
        rows.append((st.kind, st.pattern) + tuple(sv.route))
        saved.append(sv)
        shape, c_log = sv.out_shape, sv.out_shape[3]
    geoms = [tuple(getattr(g, n) for n, _ in g._fields_) for g in chain.wgrad_geoms(plan, saved)]
    return plan, rows, geoms


@pytest.mark.parametrize("config", sorted(BENCH_EXPECTED))
def test_benchmark_chains_keep_their_routes(config):
    pm = importlib.import_module(MODULES[config])
    with torch.device("meta"):
        E, G, D = pm.Encoder(), pm.Generator(), pm.Discriminator()
    seqs = {"E": E.layers, "G": G.layers, "dx": D.dx, "dz": D.dz, "dxz": D.dxz}
    expected = BENCH_EXPECTED[config]
    assert sorted(expected) == sorted(seqs)
    plans = {}
    for name, (shape, c_log, rows, geoms) in expected.items():
        plans[name], got_rows, got_geoms = _walk(seqs[name], shape, c_log)
        assert got_rows == rows, (config, name)
        assert got_geoms == geoms, (config, name)
    # D's joint rows are [dx | dz]: what the stepper asks the plans for is what dxz was recorded with
    assert plans["dx"].out_channels + plans["dz"].out_channels == expected["dxz"][0][3]
    assert plans["E"].out_channels == expected["dz"][0][3] and plans["G"].out_channels == 1


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_synthetic_stacks_reach_the_other_routes(name):
    make, shape, c_log = SYNTHETIC[name]
    with torch.device("meta"):
        seq = make()
    _, rows, geoms = _walk(seq, shape, c_log)
    assert (rows, geoms) == SYNTHETIC_EXPECTED[name]


def test_new_stacks_keep_their_routes_and_shapes():
    """the stacks test_gpu_chain_stacks.py adds to SYNTHETIC: Route rows (``_walk``) and stage shapes (``chain.trace``)"""
    from ali_hip import chain
    from chain_stacks import NEW_STACKS
    assert sorted(NEW_STACKS) == sorted(NEW_EXPECTED)
    for name, (make, shape, c_log) in NEW_STACKS.items():
        with torch.device("meta"):
            seq = make()
        plan, rows, _ = _walk(seq, shape, c_log)
        want_rows, want_shapes = NEW_EXPECTED[name]
        assert rows == want_rows, name
        traced = chain.trace(plan, shape, c_log)
        assert [traced[0][0]] + [t[1] for t in traced] == want_shapes, name
        assert [(st.kind, st.pattern) + tuple(t[2]) for st, t in zip(plan.stages, traced)] == want_rows, name


def test_every_route_value_is_pinned_somewhere():
    """the two tables together name every path ``route`` can return"""
    rows = [r for chains in BENCH_EXPECTED.values() for c in chains.values() for r in c[2]]
    rows += [r for rows_, _ in SYNTHETIC_EXPECTED.values() for r in rows_]
    assert {r[2] for r in rows} == {"head", "tconv1", "scatter", "scatter_gemm", "convT", "conv"}
    assert {r[3][0] for r in rows} | {r[4][0] for r in rows} == {
        "head", "first_direct", "conv", "tconv1", "convT_scatter", "convT", "linear", "linear_repack"}
    assert {r[3][1] for r in rows} == {"fused", "colsum", "unflat", None}
    assert {r[5] for r in rows} == {"tconv1", "convT", "conv"} and {r[6] for r in rows} == {"direct", "scatter", None}
    assert any(r[3] != r[4] for r in rows) and any(r[3][0] == r[4][0] == "first_direct" for r in rows)
