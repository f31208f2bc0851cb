"""`python SNN_DAE.py [advertiser]` -- the SNN-DAE script on MI355X.

Follows the reference's python/SNN_DAE.py: the SNN fine-tune loop of SNN_RBM.py (embedding-bag +
sigmoid input layer, three-layer MLP with dropout rows, per-example row updates -- all HIP kernels
of FNNEngine's bag mode) on top of layer-wise denoising-autoencoder pre-training
(`sampling_based_denosing_autoencoder.get_da_weights`, HIP kernels behind include/dae_hip.h),
cached in `dropda_<adv>_.p`.  Environment variables as SNN_RBM.py, and DEEPCTR_DAE_BATCH (default 1)
and DEEPCTR_DAE_CORRUPTION (default 0): the mini-batch size and corruption level of the dense
autoencoders (`get_da_weights(da_batch_size=, corruption_level=)`; the defaults are the reference's call).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deep_ctr_amd  # noqa: E402,F401
from deep_ctr_amd import SNN_RBM  # noqa: E402


def _pretrain_kw():
    return dict(da_batch_size=int(os.environ.get('DEEPCTR_DAE_BATCH', 1)),
                corruption_level=float(os.environ.get('DEEPCTR_DAE_CORRUPTION', 0)))


def run(argv):
    return SNN_RBM.run(argv, kind='dae', pretrain_kw=_pretrain_kw())


def run_many(argv, specs, out=None):
    """SNN_RBM.run_many with the denoising-autoencoder pre-trainer: every 'LR:DROPOUT:LAMBDA1' of `specs` in one pass."""
    return SNN_RBM.run_many(argv, specs, kind='dae', pretrain_kw=_pretrain_kw(), out=out)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'many':           # python SNN_DAE.py many <advertiser> LR:DROPOUT:LAMBDA1 ...
        run_many([sys.argv[0]] + sys.argv[2:3], sys.argv[3:])
    else:
        run(sys.argv)
