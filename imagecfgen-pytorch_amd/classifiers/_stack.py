"""What the three classifier files share: the ``nn.Sequential`` base that hands CUDA batches to ``ali_hip.chain``, the
layer recipe, and the training / validation loops over a spectrogram data source."""
import torch
import torch.nn as nn


class ClassifierStack(nn.Sequential):
    """An ``nn.Sequential`` whose modules own the parameters in the reference layouts (``state_dict`` keys
    ``0.weight``, ``0.bias``, ``2.weight`` ...).  CUDA batches run on the HIP kernels as one autograd node (input
    gradient included: the counterfactual explainers differentiate the classifier with respect to its image); CPU
    batches run the stock modules."""

    def forward(self, x):
        if not x.is_cuda:
            return super().forward(x)
        from ali_hip.chain import run_chain
        from ali_hip.classify import nhwc_input
        return run_chain(self, nhwc_input(x), x.shape[1]).reshape(x.shape[0], -1)


def conv_layers(widths, strides):
    """Conv2d(3x3, unpadded) + LeakyReLU(0.2) per entry, one input channel in front"""
    mods, c_in = [], 1
    for c_out, s in zip(widths, strides):
        mods += [nn.Conv2d(c_in, c_out, (3, 3), (s, s)), nn.LeakyReLU(0.2)]
        c_in = c_out
    return mods


def progress(it, total=None):
    try:
        from tqdm import tqdm
    except ImportError:
        return it
    return tqdm(it, total=total)


def make_stepper(model, l_rate):
    """the device's training step: ``ali_hip.classify.ClassifierStepper`` (HIP-graph replay on CUDA)"""
    from ali_hip.classify import ClassifierStepper
    return ClassifierStepper(model, lr=l_rate, capture=next(model.parameters()).is_cuda)


def spect_to_img_fn(mean, std, stds_kept=3):
    def spect_to_img(spect):
        return torch.clip((spect - mean) / (std + 1e-6), -stds_kept, stds_kept) / float(stds_kept)
    return spect_to_img


def accuracy_on_stream(model, batches, label_of, to_img, hw, device):
    """``n_correct / n_total`` of ``model`` over ``batches`` (audio_mnist.py:213-222), the hits kept on the device"""
    from ali_hip.classify import ClassifierScorer
    scorer = ClassifierScorer({"y": model}, capture=torch.device(device).type == "cuda")
    for batch in batches:
        scorer.add(to_img(batch["audio"]).reshape((-1, 1) + tuple(hw)), {"y": label_of(batch)})
    return scorer.result()["y"]


def train_on_source(model, data, label_of, hw, train_kwargs, valid_kwargs, epochs, l_rate, device):
    """The loop the spectrogram classifiers share (audio_mnist.py:239-291, whalecalls.py:263-323): statistics pass,
    ``spect_to_img``, Adam(lr) on CrossEntropyLoss, validation accuracy per epoch."""
    from image_scms._spect import spectrogram_statistics
    mean, std, n_batches = spectrogram_statistics(lambda: data.stream(**train_kwargs), device, clamp_variance=True)
    to_img = spect_to_img_fn(mean, std)
    stepper = make_stepper(model, l_rate)
    for e in range(epochs):
        model.train()
        loss = hits = seen = 0
        for batch in progress(data.stream(**train_kwargs), total=n_batches):
            y = label_of(batch).float()
            r = stepper.step(to_img(batch["audio"]).reshape((-1, 1) + tuple(hw)), y)
            loss, hits, seen = loss + r["loss"], hits + r["hits"], seen + len(y)      # on the device: one read per epoch
        acc = accuracy_on_stream(model, data.stream(**valid_kwargs), label_of, to_img, hw, device)
        print(f"Epoch {e + 1}/{epochs} complete. loss = {float(loss) / max(n_batches, 1):.4f} "
              f"acc = {float(hits) / max(seen, 1):.4f} Validation accuracy = {round(acc, 4)}")
    return model
