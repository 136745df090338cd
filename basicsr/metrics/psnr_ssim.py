from codeformer_amd.metrics import calculate_psnr, calculate_ssim, psnr_batch, ssim_batch  # noqa: F401
