"""Identity augmenters with imgaug's call signature: aug(images=batch) returns the batch unchanged."""


class _Identity:
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, images=None, **kwargs):
        return images


Sequential = Sometimes = GaussianBlur = AdditiveGaussianNoise = Dropout = Multiply = LinearContrast = Grayscale = _Identity
ElasticTransformation = _Identity
