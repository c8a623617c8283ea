"""Numbers that both the input side (data/) and the predictor use: a leaf module, so neither has to import the other for them."""

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
