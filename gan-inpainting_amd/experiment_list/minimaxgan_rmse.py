"""Plugin `minimaxgan_rmse`: begin(state, loaders), the contract of the reference's train.py:183-186.
Schedule: experiment_list/minimaxgan_rmse.py:110-173 of the reference (minimax GAN, BCE adversarial loss +
RMSE reconstruction, Adam lr=2e-4 betas=(0.5,0.999)), executed by trainer.MinimaxStep on the HIP backend."""
from . import _common as C


def begin(state, loaders):
    state, exp_dir, logger, device = C.setup(state, "minimaxgan_rmse")
    C.refuse_lpips_loss(state, "minimaxgan_rmse")
    net_G, (net_D,) = C.build_networks(state, device, n_disc=1, sigmoid=True)
    opt_G, opt_D = C.make_optimizers("adam", net_G, net_D.parameters())
    step = C.trainer.MinimaxStep(net_G, net_D, opt_G, opt_D, recon="rmse", sync=C.make_sync(), diffaug=C.make_diffaug(state))
    step.ema_G = C.make_ema(state, net_G)

    def batch(bi, ground, mask):
        return step(ground, mask), True

    return C.run_epochs(state, loaders, exp_dir, logger, device, net_G, [net_D], batch, ["avg_d"], step=step)
