"""vaenmf: MI355X-native engine for the VAE-NMF reconstruct path."""
from . import _lib
from .models import VariationalAutoencoder, DeepGenerativeModel, Classifier, Classifier2Classes, Encoder, Decoder
from .mcem import MCEM_M1, MCEM_M2, EM_noNMF, MCEM_M2_noNMF
from .engine import BatchEngine
from .resample import resample, resample_batch
from .dataset import FeatureMoments, make_test_set, make_train_set, mix_batch, plan_mixes
from .train import Trainer, fit_classifier, fit_m1, fit_m2
from .train_mask import MaskTrainer, fit_mask_filter, mask_spec
