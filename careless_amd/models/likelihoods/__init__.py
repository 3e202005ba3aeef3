from careless_amd.models.likelihoods.mono import NeuralLikelihood, NeuralNormalLikelihood  # noqa: F401
