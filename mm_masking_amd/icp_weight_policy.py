"""``LearnICPWeightPolicy`` — host-side mirror of the reference module
``mm_masking/icp_weight_policy.py`` (same constructor ``params`` keys, same
``forward``/``icp`` signatures and return values, same ``state_dict`` keys), with

  * the mask U-Net in hand-written NHWC bf16 MFMA kernels (unet_hip.py ->
    csrc/mmk_unet.hip): ReLU (the reference's default) and LeakyReLU(0.1)
    (``params["leaky"]``) networks, with or without BatchNorm (``params["batch_norm"]``,
    unet_hip_bn.py), Cartesian or polar input of any size >= 32 x 32.
    There is no vendor-library (MIOpen) or CPU fallback on a HIP device; the
    ``nn.Module`` tree is the parameter store (identical ``state_dict``) and, with the
    explicit ``unet_backend="torch"`` on a CPU device, the host-logic mirror the CPU
    tests compare with the reference's golden vectors,
  * ``extract_weights`` and the differentiable ICP in hand-written HIP kernels
    (radar_utils.py / dICP/ICP.py of this package -> libmmk_hip.so).

Reference lines: constructor :25-102, conv_block :104-125, forward :127-275,
icp :277-288.  The Neptune/matplotlib plotting block (:221-264) is observability
SaaS and out of scope: ``neptune_run``, ``epoch`` and ``batch_idx`` are accepted
and ignored.  The per-step ``torch.cuda.empty_cache()`` calls (:187,217) are not
reproduced (they only force syncs).
"""
import torch
import torch.nn as nn
from torch.nn import ModuleList

from . import _lib
from .dICP.ICP import ICP
from .radar_utils import (_extract_weights_polar_stats, _extract_weights_stats, cfar_mask, deskew_pc, extract_pc_padded, extract_weights,
                          form_cart_range_angle_grid, form_polar_range_grid, mask_polar_scan, scan_times)


def weights_init(m):
    """icp_weight_policy.py:15-22."""
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        try:
            nn.init.xavier_uniform_(m.weight.data)
            nn.init.zeros_(m.bias)
        except AttributeError:
            print("Skipping initialization of ", classname)


def _global_extrema(c_min, c_max):
    """min / max over the ranks of a data-parallel job (one MAX all-reduce of [-min, max]); the identity in a
    single-process run.  Same reduction as unet_hip.channel_minmax(global_reduce=True) on the HIP path."""
    from .ddp import dist, job_size
    if job_size() == 1:
        return c_min, c_max
    t = torch.stack((-c_min.detach(), c_max.detach()))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return -t[0], t[1]


# scan mode and polar sampling: how the option reads in a message, the params setting that makes prepare_batch supply what
# it reads, and what it does in a HIP kernel
_BATCH_OPTIONS = {"scan": ("mask_target='scan'", "params['mask_target'] = 'scan'", "runs the radar front end in HIP kernels"),
                  "polar": ("polar_sampling", "params['polar_sampling'] = True", "samples the mask in a HIP kernel")}


def _check_batch(option, batch_scan, keys, device=None):
    """What a forward with ``option`` needs: ``keys`` in batch_scan and, when ``device`` is given, a HIP device."""
    what, setting, does = _BATCH_OPTIONS[option]
    for key in keys:
        if key not in batch_scan:
            raise KeyError("%s needs batch_scan[%r] (prepare_batch with %s, or finish_batch(keep_polar=True))" % (what, key, setting))
    if device is not None and torch.device(device).type != "cuda":
        raise _lib.MmkError("%s %s with no CPU path: params['device'] must be a HIP device" % (what, does))


class LearnICPWeightPolicy(nn.Module):
    def __init__(self, params):
        super().__init__()
        self.res = 0.0596

        icp_type = params["icp_type"]
        network_inputs = {"fft": params["fft_input"], "cfar": params["cfar_input"], "range": params["range_input"]}
        network_input_type = params["network_input_type"]
        device = params["device"]
        max_iter = params["max_iter"]

        self.use_ICP_4_train = params["loss_icp_rot_weight"] > 0.0 and params["loss_icp_trans_weight"] > 0.0

        config_path = "../external/dICP/config/dICP_config.yaml"
        self.ICP_alg = ICP(icp_type=icp_type, config_path=config_path, differentiable=True,
                           max_iterations=max_iter, tolerance=1e-5)
        self.ICP_alg_inference = ICP(icp_type=icp_type, config_path=config_path, differentiable=False,
                                     max_iterations=50, tolerance=1e-5)
        self.float_type = params["float_type"]
        self.device = device
        self.network_inputs = network_inputs
        if network_input_type == "cartesian":
            self.range_mask, _ = form_cart_range_angle_grid(device=device)
        elif network_input_type == "polar":
            self.range_mask = form_polar_range_grid(polar_resolution=self.res, device=device)

        self.network_input_type = network_input_type
        self.network_output_type = params["network_output_type"]
        self.leaky = params["leaky"]
        self.dropout = params["dropout"]
        self.batch_norm = params["batch_norm"]
        self.normalize_type = params["normalize"]
        self.log_transform = params["log_transform"]
        self.a_thres = params["a_thresh"]
        self.b_thres = params["b_thresh"]
        self.gt_eye = params["gt_eye"]
        self.norm_weights = params["norm_weights"]

        # optional keys (absent upstream): what the reference hard-codes in icp()
        self.icp_loss_fn = params.get("icp_loss_fn", {"name": "cauchy", "metric": 1.0})
        self.icp_trim_dist = params.get("icp_trim_dist", 5.0)
        self.icp_dim = params.get("icp_dim", 2)
        # params["icp_trim"] / ["icp_tanh_steepness"] (absent upstream): the trim gate of the TRAINING instance, "hard" or the
        # soft "tanh" gate that the backward differentiates (dICP/ICP.py); the inference instance keeps the hard gate
        self.icp_trim = params.get("icp_trim", "hard")
        if self.icp_trim not in ("hard", "tanh"):
            raise ValueError("icp_trim must be 'hard' or 'tanh' (got %r)" % (self.icp_trim,))
        steep = params.get("icp_tanh_steepness", 10.0)
        if isinstance(steep, bool) or not isinstance(steep, (int, float)) or not (0.0 < float(steep) < float("inf")):
            raise ValueError("icp_tanh_steepness must be a finite number > 0 (got %r)" % (steep,))
        self.icp_tanh_steepness = float(steep)
        if "icp_trim" in params:                    # (absent: whatever the dICP configuration says, "hard" by default)
            self.ICP_alg.trim = self.icp_trim
        if "icp_tanh_steepness" in params:
            self.ICP_alg.tanh_steepness = self.icp_tanh_steepness
        self.ICP_alg_inference.trim = "hard"
        # params["icp_correspondence"] / ["icp_softmin_k"] / ["icp_softmin_temp"] (absent upstream): the correspondences of the
        # TRAINING instance, "nearest" or the "softmin" over the k nearest target rows that the backward differentiates
        # (dICP/ICP.py); the inference instance keeps nearest correspondences.  Works with mask_target="scan" (that mode
        # runs unweighted: the mask acts through the points); of learn_icp's names it combines with "softmin_temp" only (the
        # other three are tensor hyper-parameters of the hard-correspondence entries).
        self.icp_correspondence = params.get("icp_correspondence", "nearest")
        if self.icp_correspondence not in ("nearest", "softmin"):
            raise ValueError("icp_correspondence must be 'nearest' or 'softmin' (got %r)" % (self.icp_correspondence,))
        learn = params.get("learn_icp", ()) or ()
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        if self.icp_correspondence == "softmin" and any(name != "softmin_temp" for name in learn):
            raise ValueError("icp_correspondence='softmin' does not combine with learn_icp (tensor hyper-parameters)")
        if "softmin_temp" in learn and self.icp_correspondence != "softmin":
            raise ValueError("learn_icp: 'softmin_temp' needs icp_correspondence='softmin': nearest correspondences have no "
                             "temperature")
        if "icp_correspondence" in params:          # (absent: whatever the dICP configuration says, "nearest" by default)
            self.ICP_alg.correspondence = self.icp_correspondence
        if "icp_softmin_k" in params:
            self.ICP_alg.softmin_k = params["icp_softmin_k"]
        if "icp_softmin_temp" in params:
            self.ICP_alg.softmin_temp = params["icp_softmin_temp"]
        self.ICP_alg._softmin()                     # validates k (2..8) and the temperature (> 0): ValueError
        self.icp_softmin_k, self.icp_softmin_temp = self.ICP_alg.softmin_k, self.ICP_alg.softmin_temp
        self.ICP_alg_inference.correspondence = "nearest"
        # "hip" (the product path): hand-written NHWC bf16 kernels (csrc/mmk_unet.hip), fp32 masters;
        # "torch": the nn.Module tree evaluated by PyTorch on the CPU -- host-logic mirror for tests only
        self.unet_backend = params.get("unet_backend", "hip")
        if self.unet_backend not in ("hip", "torch"):
            raise ValueError("unet_backend must be 'hip' or 'torch' (got %r)" % (self.unet_backend,))
        # what the mask acts on.  "weights" (default, the reference's forward): the mask is sampled at the fixed CFAR cloud and
        # weighs its points in ICP.  "scan": the mask multiplies the polar scan (the reference's comment at
        # icp_weight_policy.py:266), the cloud is extracted again from the masked scan with the differentiable front end, and
        # ICP runs unweighted on it -- the mask acts through the points.
        self.mask_target = params.get("mask_target", "weights")
        if self.mask_target not in ("weights", "scan"):
            raise ValueError("mask_target must be 'weights' or 'scan' (got %r)" % (self.mask_target,))
        # params["polar_sampling"] (absent upstream): a polar network's mask is sampled where the points lie in the polar image
        # (radar_utils.extract_weights_polar) instead of with point_to_cart_idx's Cartesian normalisation, the reference's
        # latent bug that the default keeps.  forward then reads batch_scan["azimuths"].
        self.polar_sampling = bool(params.get("polar_sampling", False))
        if self.polar_sampling and network_input_type != "polar":
            raise ValueError("polar_sampling needs network_input_type='polar': a Cartesian mask is sampled on its own grid already")
        if self.polar_sampling and self.mask_target != "weights":
            raise ValueError("polar_sampling needs mask_target='weights': the scan mode does not weigh points with the mask")
        # data-parallel jobs: reduce the min-max normalisation's extrema over the ranks (one MAX all-reduce of 2C floats), so
        # that it stays global over the whole batch as in the single-process reference (icp_weight_policy.py:151-155).
        # Default: ON whenever the process is a rank of a multi-rank job, so that N ranks x B pairs normalise like one
        # process over N*B pairs; params["global_minmax"] = False keeps it per rank.  The default is resolved at forward
        # time (the ``global_minmax`` property), so a model built before init_process_group normalises globally too.
        # The reduction is a COLLECTIVE: every rank must run the same number of forwards (training and validation
        # alike) -- train_icp_weights.fit() validates on all ranks for this reason.
        # params["motion_comp"] (absent upstream, whose filtered_pc arrives motion-compensated): in the scan mode the cloud that
        # is extracted from the masked scan is de-skewed with the constant twist batch_scan["velocity"] (B,6) = (v; omega) in
        # m/s and rad/s before ICP (radar_utils.deskew_pc).  batch_scan["az_times"] holds the azimuth stamps
        # in multiples of params["motion_time_unit"] seconds (1e-6: synthetic's stamps); params["motion_ref"] names the time
        # the pose refers to ("mid", "first" or "last", radar_utils.scan_times).
        self.motion_comp = bool(params.get("motion_comp", False))
        self.motion_time_unit = float(params.get("motion_time_unit", 1e-6))
        self.motion_ref = params.get("motion_ref", "mid")
        if self.motion_ref not in ("mid", "first", "last"):
            raise ValueError("motion_ref must be 'mid', 'first' or 'last' (got %r)" % (self.motion_ref,))
        gm = params.get("global_minmax", None)
        self._global_minmax = None if gm is None else bool(gm)
        self._step = 0

        self.mean_num_pts = 0.0
        self.max_w = 0.0
        self.min_w = 0.0
        self.mean_w = 0.0
        self.mean_all_pts = 0.0
        self.mean_scan_pts = 0.0          # scan mode: mean number of points extracted from the masked scan (device tensor)

        init_c_num = network_inputs["fft"] + network_inputs["cfar"] + network_inputs["range"]
        enc_channels = [init_c_num, 8, 16, 32, 64, 128, 256]
        dec_channels = [256, 128, 64, 32, 16, 8]
        self.encoder = ModuleList([self.conv_block(enc_channels[i], enc_channels[i + 1], i)
                                   for i in range(len(enc_channels) - 1)])
        self.decoder = ModuleList([self.conv_block(dec_channels[i], dec_channels[i + 1])
                                   for i in range(len(dec_channels) - 1)])
        self.final_layer = nn.Sequential(nn.Conv2d(dec_channels[-1], 1, kernel_size=1), nn.Sigmoid())
        if params["init_weights"]:
            self.apply(weights_init)
        # params["learn_cfar"] (absent upstream): the two GO-CFAR thresholds of the scan mode's detector become parameters,
        # trained with the mask through cfar_mask's threshold gradients.  They start from params["a_thresh"] / ["b_thresh"];
        # the CFAR input channel (computed with diff=False by the dataset / prepare_batch) keeps those fixed values.
        self.learn_cfar = bool(params.get("learn_cfar", False))
        if self.learn_cfar:
            if self.mask_target != "scan":
                raise ValueError("learn_cfar needs mask_target='scan': the default mode never runs the detector in its forward")
            self.cfar_a = nn.Parameter(torch.tensor(float(self.a_thres), dtype=torch.float32))
            self.cfar_b = nn.Parameter(torch.tensor(float(self.b_thres), dtype=torch.float32))
        # params["learn_icp"] (absent upstream): names out of ("metric", "trim_dist", "tanh_steepness") whose value inside
        # the ICP becomes a scalar parameter (one value for the batch), read by the training instance on the device and
        # trained through the ICP's hyper-parameter gradients (dICP/ICP.py).  They start from icp_loss_fn["metric"],
        # icp_trim_dist and icp_tanh_steepness.  Nothing keeps a learned value in range: the ICP's status flag reports one
        # that left it.  "softmin_temp" (with icp_correspondence="softmin", checked above): the soft-min temperature becomes
        # the scalar parameter icp_softmin_temp_p, started from icp_softmin_temp and trained through the ICP's temperature
        # gradient (DESIGN.md §3 I7⁗); the inference instance keeps nearest correspondences and never reads it.
        learn_icp = params.get("learn_icp", ())
        if isinstance(learn_icp, str):
            learn_icp = (learn_icp,)
        self.learn_icp = tuple(learn_icp)
        for name in self.learn_icp:
            if name not in ("metric", "trim_dist", "tanh_steepness", "softmin_temp"):
                raise ValueError("learn_icp: unknown name %r (choose from 'metric', 'trim_dist', 'tanh_steepness', 'softmin_temp')"
                                 % (name,))
            if name in ("trim_dist", "tanh_steepness") and self.icp_trim != "tanh":
                raise ValueError("learn_icp: %r needs icp_trim='tanh': the hard gate is a constant of the backward" % (name,))
            if name == "metric" and (self.icp_loss_fn is None or self.icp_loss_fn.get("name") not in
                                     ("cauchy", "huber", "geman_mcclure", "welsch")):
                raise ValueError("learn_icp: 'metric' needs a robust loss (icp_loss_fn name 'cauchy', 'huber', "
                                 "'geman_mcclure' or 'welsch')")
        if "metric" in self.learn_icp:
            self.icp_metric = nn.Parameter(torch.tensor(float(self.icp_loss_fn.get("metric", 1.0)), dtype=torch.float32))
        if "trim_dist" in self.learn_icp:
            self.icp_trim_dist_p = nn.Parameter(torch.tensor(float(self.icp_trim_dist), dtype=torch.float32))
        if "tanh_steepness" in self.learn_icp:
            self.icp_tanh_steepness_p = nn.Parameter(torch.tensor(self.icp_tanh_steepness, dtype=torch.float32))
        if "softmin_temp" in self.learn_icp:
            self.icp_softmin_temp_p = nn.Parameter(torch.tensor(float(self.icp_softmin_temp), dtype=torch.float32))

    @property
    def global_minmax(self):
        """Whether the min-max extrema are reduced over the ranks: the explicit params["global_minmax"] / assigned value,
        else "this process is a rank of a multi-rank job" -- asked when used, not when the model was built."""
        if self._global_minmax is not None:
            return self._global_minmax
        from .ddp import job_size
        return job_size() > 1

    @global_minmax.setter
    def global_minmax(self, value):
        self._global_minmax = None if value is None else bool(value)

    def conv_block(self, in_channels, out_channels, i=0):
        """icp_weight_policy.py:104-125 (module order fixes the state_dict keys)."""
        relu_layer = nn.LeakyReLU(0.1) if self.leaky else nn.ReLU()
        modules = [nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1), relu_layer]
        if self.batch_norm:
            modules.append(nn.BatchNorm2d(out_channels))
        modules.append(nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1))
        modules.append(relu_layer)
        if self.batch_norm:
            modules.append(nn.BatchNorm2d(out_channels))
        if self.dropout > 0.0:
            modules.append(nn.Dropout(p=self.dropout))
        if i > 0:
            modules.append(nn.MaxPool2d(kernel_size=2, stride=2))
        return nn.Sequential(*modules)

    # ------------------------------------------------------------------ U1-U4
    def _network_input(self, fft_data, fft_cfar, normalize=True):
        """icp_weight_policy.py:136-159.  ``normalize=False`` stops before the per-channel normalisation
        (the hand-written first layer applies the min-max form while it loads the image)."""
        input_data = None
        if self.network_inputs["fft"]:
            input_data = fft_data.unsqueeze(1)
        if self.network_inputs["cfar"]:
            input_data = torch.cat([input_data, fft_cfar.unsqueeze(1)], dim=1)
        if self.network_inputs["range"]:
            rm = self.range_mask.to(input_data.device)
            range_stack = rm.unsqueeze(0).expand(input_data.shape[0], -1, -1).unsqueeze(1)
            input_data = torch.cat([input_data, range_stack], dim=1)
        if self.log_transform:
            input_data = torch.log(input_data + 1e-6)
        if not normalize:
            return input_data
        return self._normalize_channels(input_data)

    def _normalize_channels(self, input_data):
        chans = []
        for c in range(input_data.shape[1]):
            xc = input_data[:, c, :, :]
            if "minmax" in self.normalize_type:
                c_max, c_min = torch.max(xc), torch.min(xc)
                if self.global_minmax:
                    c_min, c_max = _global_extrema(c_min, c_max)
                xc = (xc - c_min) / (c_max - c_min)
            elif "standardize" in self.normalize_type:
                xc = (xc - torch.mean(xc)) / torch.std(xc)
            chans.append(xc)
        return torch.stack(chans, dim=1)

    def _unet(self, input_data):
        """icp_weight_policy.py:161-184 through the nn.Module tree (fp32, CPU: tests only)."""
        enc_layers = []
        for layer in self.encoder:
            enc_layers.append(input_data)
            input_data = layer(input_data)
        enc_layers.reverse()
        for i, decoder_layer in enumerate(self.decoder):
            skip_con = enc_layers[i]
            input_data = nn.functional.interpolate(input_data, size=(skip_con.shape[2], skip_con.shape[3]),
                                                   mode="bilinear", align_corners=True)
            input_data = decoder_layer(input_data)
            input_data = torch.cat([skip_con, input_data], dim=1)
            input_data = decoder_layer(input_data)   # same weights applied twice (:178,182)
        logits = self.final_layer[0](input_data)
        return torch.sigmoid(logits.float()).squeeze(1)

    def _unet_hip(self, raw_in):
        """The mask of the raw network input (B, C, H, W) from the hand-written kernels (unet_hip.py / unet_hip_bn.py), with
        the per-channel normalisation folded into the first layer's loads and, with norm_weights, the amax normalisation of
        the mask inside the same autograd node."""
        from . import unet_hip, unet_hip_bn
        if not raw_in.is_cuda:
            raise _lib.MmkError("the mask U-Net is a set of HIP kernels with no CPU path: params['device'] must be "
                                "a HIP device (unet_backend='torch' is the CPU host-logic mirror used by tests)")
        # any image of at least 32 x 32 (five floor-rounding poolings leave >= 1 pixel): the Cartesian
        # 640 x 640 grid and the polar 400 x 3360 one (network_input_type "polar") alike
        if raw_in.shape[1] > 4 or raw_in.shape[2] < 32 or raw_in.shape[3] < 32:
            raise _lib.MmkError("mask U-Net: unsupported network input %s (1..4 channels, at least 32 x 32)"
                                % (tuple(raw_in.shape),))
        self._step += 1
        # an image that requires grad receives its gradient from the network's autograd node; the statistics of a
        # folded normalisation are computed outside the graph, so the node is told which ones they are (input_norm)
        want_gx = torch.is_grad_enabled() and raw_in.requires_grad
        mode = next((m for m in ("minmax", "standardize") if m in self.normalize_type), None)
        if mode is None:
            net_in, pre, mm = self._normalize_channels(raw_in), None, None
        else:
            # folded into the first layer's loads: one pass for (min, max), or two ordered ones for (mean, 1 / std) -- per
            # rank under data parallelism, as the reference's torch.mean / torch.std of its own batch -- and no
            # normalised copy of the image
            net_in = raw_in.contiguous().float()
            if mode == "standardize":
                pre, mm = unet_hip.channel_meanstd(net_in), None
            elif not want_gx:
                pre, mm = unet_hip.channel_minmax(net_in, global_reduce=self.global_minmax), None
            elif unet_hip.minmax_is_collective(self.global_minmax):
                raise _lib.MmkError("the gradient with respect to the network input through min-max extrema that are "
                                    "reduced over the ranks is not implemented: set params['global_minmax'] = False "
                                    "or detach the input")
            else:
                pre, mm = unet_hip.channel_minmax(net_in, return_minmax=True)
        # batch_norm: Conv, ReLU, BN, Conv, ReLU, BN, with BatchNorm kernels between the convolutions
        return (unet_hip_bn if self.batch_norm else unet_hip).unet_mask(
            self, net_in, self.training, self._step, norm=self.norm_weights, pre=pre, slope=0.1 if self.leaky else 0.0,
            input_norm=(mode, mm) if want_gx and mode is not None else None)

    def forward(self, batch_scan, batch_map, T_init, binary=False, override_mask=None, neptune_run=None, epoch=0,
                batch_idx=0, mask_only=False):
        if self.motion_comp and self.mask_target == "scan" and not mask_only:      # (before anything touches the device)
            for key in ("velocity", "az_times"):
                if batch_scan.get(key) is None:
                    raise ValueError("motion_comp needs batch_scan[%r] (prepare_batch with params['motion_comp'] = True on "
                                     "pairs that carry a velocity)" % key)
        fft_data = batch_scan["fft_data"].to(self.device)
        fft_cfar = batch_scan["fft_cfar"].to(self.device)
        scan_pc_raw = batch_scan["raw_pc"].to(self.device)
        map_pc = batch_map["pc"].to(self.device)
        if self.mask_target == "scan" and not mask_only:
            _check_batch("scan", batch_scan, ("azimuths",) if self.network_input_type == "polar" else ("fft_polar", "azimuths"),
                         self.device)
        if self.polar_sampling and not mask_only:
            _check_batch("polar", batch_scan, ("azimuths",), self.device)
            n_az = batch_scan["azimuths"].shape[1]
            if override_mask is not None and (override_mask.ndim != 3 or override_mask.shape[0] != scan_pc_raw.shape[0] or
                                              override_mask.shape[1] != n_az):
                raise ValueError("polar_sampling: override_mask must be a polar (B, %d, R) mask (got %s)"
                                 % (n_az, tuple(override_mask.shape)))

        normalised = False
        if override_mask is not None:
            weight_mask = override_mask.to(self.device)
        else:
            raw_in = self._network_input(fft_data, fft_cfar, normalize=False)
            if self.unet_backend == "hip":
                weight_mask = self._unet_hip(raw_in)
                normalised = self.norm_weights      # (the amax normalisation rides inside the network's autograd node)
            elif raw_in.is_cuda:
                raise _lib.MmkError("unet_backend='torch' is the CPU host-logic mirror (tests only); on a HIP device "
                                    "the U-Net runs on the hand-written kernels (unet_backend='hip')")
            else:
                weight_mask = self._unet(self._normalize_channels(raw_in))

        if self.norm_weights and not normalised:
            weight_mask = weight_mask / torch.amax(weight_mask, dim=(1, 2), keepdim=True)
        if binary:
            weight_mask = torch.where(weight_mask > 0.5, 1.0, 0.0)
        if mask_only:
            return weight_mask

        if self.polar_sampling:
            (weights, diff_mean_num_non0, mean_num_non0, mean_w, max_w, min_w), stats = \
                _extract_weights_polar_stats(weight_mask, scan_pc_raw, batch_scan["azimuths"], self.res)
        else:
            (weights, diff_mean_num_non0, mean_num_non0, mean_w, max_w, min_w), stats = \
                _extract_weights_stats(weight_mask, scan_pc_raw)
        self.mean_num_pts = mean_num_non0
        self.max_w = max_w
        self.min_w = min_w
        self.mean_w = mean_w
        # points with x != 0 and y != 0, per scan (icp_weight_policy.py:209-212): same fused pass
        self.mean_all_pts = stats[5]

        if self.mask_target == "scan":
            return self._forward_scan(batch_scan, map_pc, T_init, weight_mask, scan_pc_raw.shape[1]), weight_mask, \
                diff_mean_num_non0

        scan_pc_filt = batch_scan["filtered_pc"].to(self.device)

        if self.training and not self.use_ICP_4_train:
            return T_init, weight_mask, diff_mean_num_non0

        T_est = self.icp(scan_pc_filt, map_pc, T_init, weights)
        return T_est, weight_mask, diff_mean_num_non0

    def _forward_scan(self, batch_scan, map_pc, T_init, weight_mask, max_pts):
        """mask_target="scan": mask -> masked polar scan -> GO-CFAR -> blob centres -> unweighted ICP, every link with its
        hand-written backward.  diff=True in training and evaluation alike, so both see the same cloud.  With
        params["learn_cfar"] the detector reads its thresholds from the parameters cfar_a / cfar_b on the device."""
        azimuths = batch_scan["azimuths"]
        if self.network_input_type == "polar":          # the mask is polar already
            masked = weight_mask * batch_scan["fft_data"].to(self.device)
        else:
            # (host azimuths cost no synchronisation: the operator forms their sin / cos on the host)
            masked = mask_polar_scan(batch_scan["fft_polar"].to(self.device), weight_mask, azimuths, self.res)
        a_th, b_th = (self.cfar_a, self.cfar_b) if self.learn_cfar else (self.a_thres, self.b_thres)
        m = cfar_mask(masked, self.res, a_thresh=a_th, b_thresh=b_th, diff=True)
        az = azimuths.to(self.device)
        az_times = batch_scan.get("az_times")
        az_times = torch.zeros_like(az) if az_times is None else az_times.to(self.device)
        if self.motion_comp:
            # (forward has checked the two keys)  The extracted cloud lies where the image shows it; ICP gets it de-skewed.
            # batch_scan["velocity"] may require grad: it receives the ICP's source-cloud gradient through deskew_pc.
            seconds = scan_times(az_times, self.motion_time_unit, self.motion_ref)
            cloud, cnt, t = extract_pc_padded(m, self.res, az, seconds, max_pts=max_pts, diff=True, return_times=True)
            cloud = deskew_pc(cloud, t, batch_scan["velocity"].to(self.device))
        else:
            cloud, cnt = extract_pc_padded(m, self.res, az, az_times, max_pts=max_pts, diff=True)
        self.mean_scan_pts = cnt.float().mean()
        if self.training and not self.use_ICP_4_train:
            return T_init
        return self.icp(cloud, map_pc, T_init, None)

    def icp(self, scan_pc, map_pc, T_init, weights):
        """icp_weight_policy.py:277-288 (loss_fn / trim_dist / dim hard-coded there;
        overridable here through optional params keys)."""
        alg = self.ICP_alg if self.training else self.ICP_alg_inference
        loss_fn, trim_dist = self.icp_loss_fn, self.icp_trim_dist
        # params["learn_icp"]: the training instance reads the parameters (and trains them); the inference instance keeps
        # its hard gate and reads the learned metric and trim distance, detached -- the steepness has no meaning there
        if "metric" in self.learn_icp:
            loss_fn = dict(loss_fn, metric=self.icp_metric if self.training else self.icp_metric.detach())
        if "trim_dist" in self.learn_icp:
            trim_dist = self.icp_trim_dist_p if self.training else self.icp_trim_dist_p.detach()
        if "tanh_steepness" in self.learn_icp and self.training:
            alg.tanh_steepness = self.icp_tanh_steepness_p
        if "softmin_temp" in self.learn_icp and self.training:
            alg.softmin_temp = self.icp_softmin_temp_p
        icp_result = alg.icp(scan_pc, map_pc, T_init=T_init, weight=weights, trim_dist=trim_dist,
                             loss_fn=loss_fn, dim=self.icp_dim)
        return icp_result["T"]
