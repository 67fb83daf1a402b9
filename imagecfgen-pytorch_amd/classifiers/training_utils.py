"""``batchify`` of the reference's ``classifiers/training_utils.py`` (:1-8)."""


def batchify(*tensors, batch_size=128):
    n = min(len(t) for t in tensors)
    for lo in range(0, n, batch_size):
        yield tuple(t[lo:lo + batch_size] for t in tensors)
