"""Command-line surface of the reference (options/base_options.py:15-163,
options/train_options.py:7-40, options/test_options.py:4-14) — same flag names, types and
defaults, so scripts/mm-train-ratio.sh-style invocations parse unchanged.

Differences, all deliberate:
  * the non-distributed branch works (the reference raises AttributeError at
    base_options.py:191 by calling .split on a list);
  * --distributed reads RANK/LOCAL_RANK/WORLD_SIZE from the environment (torchrun) and
    initialises the 'nccl' backend, which is RCCL on ROCm;
  * --opt_level O0 = fp32; O1/O2 (apex AMP in the reference) = bf16 MFMA compute with fp32 master
    weights, accumulation and statistics plus apex's dynamic loss scaling (three device-resident
    scalers, skip / back off / grow); O1_FP16/O2_FP16 = the same with IEEE fp16 operands (apex's own
    numerics); BF16 = the bf16 compute without a scaler;
  * conv biases that feed an InstanceNorm get their exact (zero) gradient by default instead of the reference's
    rounding noise (ops.EXACT_NULL_BIAS_GRAD; MMH_NULL_BIAS_GRAD=compute restores it);
  * --fp32_exact_grads (addition): the gradient-exact fp32 hybrid, see ops.set_winograd_mode;
  * --fp32_exact_fwd direct | wino2 (addition): that hybrid's forward kernels (wino2 = ops.set_winograd_mode("bwd_f2"));
  * --graph_step (addition): single-process training replays the whole iteration from a captured hipGraph
    (MMHandModel._optimize_parameters_graph);
  * three additions: --G_n_blocks (the reference hard-codes 9), --vgg_weights (file with
    torchvision vgg19.features[0:4] weights; there is no download path offline) and
    --vgg_random_init (explicit opt-in to seeded random VGG weights; without either of the two
    the default --L1_type l1_plus_perL1 refuses to start);
  * --resize_inputs N (addition; 0 = off): file-fed batches (--dataroot) reach the networks at N x N whatever size the
    files hold - the resize happens inside the device's decode pass (ops.decode_inputs).  --fineSize keeps the dead
    meaning it has in the reference (declared, never read);
  * --resident_dataset / --resident_gb G (additions; off): the file-fed loader keeps the decoded dataset in device memory
    after the first epoch (data.HandFolderLoader(resident=True));
  * --pairing random | curriculum | nearest, --match_pool self | train (additions; random = the reference's live loader):
    the paper's pairing strategies on the reference's pose distance (data.HandFolderLoader, csrc/pose_knn.hip);
  * --augment_geom with --aug_rotate / --aug_scale / --aug_shift / --aug_flip / --aug_pair / --aug_seed (additions to `train`;
    off): a random affine transform per image and epoch inside the device's decode pass (data.augment_draws,
    ops.decode_inputs_affine).  The reference declares --no_flip / --use_flip and never reads them; they stay dead here;
  * --depth_source files | joints with --render_radius / --render_bg (additions; files = the reference's loader): joints
    renders D1 / D2 from C1 / C2 on the device (ops.render_pose_depth, csrc/render_depth.hip) instead of reading depth PNGs.
"""
import argparse
import os

# (flag, kwargs) tables — base, train, test
_BASE = [
    ("--imageroot", dict(type=str, help="path to images")),
    ("--poseroot", dict(type=str, help="path to poses")),
    ("--batchSize", dict(type=int, help="input batch size")),
    ("--fineSize", dict(type=int, default=256, help="then crop to this size")),
    ("--output_nc", dict(type=int, default=3, help="# of output image channels")),
    ("--ngf", dict(type=int, default=64, help="# of generator filters in first conv layer")),
    ("--ndf", dict(type=int, default=64, help="# of discrimator filters in first conv layer")),
    ("--n_layers_D", dict(type=int, default=3, help="blocks used in D")),
    ("--gpu_ids", dict(type=str, default="0", help="gpu ids: e.g. 0  0,1,2, 0,2. use -1 for CPU")),
    ("--name", dict(type=str, default="experiment_name", help="name of the experiment")),
    ("--nThreads", dict(type=int, default=8, help="# threads for loading data")),
    ("--checkpoints_dir", dict(type=str, default="./checkpoints", help="models are saved here")),
    ("--norm", dict(type=str, default="batch", help="instance normalization or batch normalization")),
    ("--serial_batches", dict(action="store_true", help="take images in order to make batches")),
    ("--display_winsize", dict(type=int, default=256, help="display window size")),
    ("--display_id", dict(type=int, default=0, help="window id of the web display")),
    ("--display_port", dict(type=int, default=8097, help="visdom port of the web display")),
    ("--no_dropout", dict(action="store_true", help="no dropout for the generator")),
    ("--max_dataset_size", dict(type=int, default=float("inf"), help="max samples per dataset")),
    ("--no_flip", dict(action="store_true", help="do not flip the images for augmentation")),
    ("--init_type", dict(type=str, default="normal", help="network initialization")),
    ("--H_input_nc", dict(type=int, default=3, help="# of input image channels")),
    ("--P_input_nc", dict(type=int, default=21, help="# of pose-map channels")),
    ("--D_input_nc", dict(type=int, default=3, help="# of depth channels")),
    ("--padding_type", dict(type=str, default="reflect", help="padding type (always reflect)")),
    ("--pairLst", dict(type=str, help="market pairs")),
    ("--use_flip", dict(type=int, default=0, help="flip or not")),
    ("--G_n_downsampling", dict(type=int, default=2, help="down-sampling blocks for generator")),
    ("--D_n_downsampling", dict(type=int, default=2, help="down-sampling blocks for discriminator")),
    ("--augmentation_ratio", dict(type=float)),
    ("--augmentation_method", dict(type=str)),
    ("--dataset_mode", dict(type=str)),
    ("--dataset", dict(type=str)),
    ("--dataroot", dict(type=str)),
    ("--local_rank", dict(type=int, default=0, help="determine which is the master process")),
    ("--distributed", dict(action="store_true", help="one process per GPU, RCCL all-reduce")),
    ("--seed", dict(type=int, default=49, help="manual seed for weight init")),
    ("--opt_level", dict(type=str, default="O0",
                         help="O0 fp32 | O1/O2 bf16 MFMA compute + dynamic loss scaling | O1_FP16/O2_FP16 the same in "
                              "IEEE fp16 | BF16 (no scaler)")),
    ("--G_n_blocks", dict(type=int, default=9, help="PATBlocks in the generator")),
    ("--vgg_weights", dict(type=str, default=None, help="vgg19.features[0:4] state_dict file")),
    ("--vgg_random_init", dict(action="store_true",
                               help="perceptual loss on seeded RANDOM VGG weights (benchmarks / tests; "
                                    "not the reference's objective)")),
    ("--fp32_exact_grads", dict(action="store_true",
                                help="fp32 only: forward 3x3 convs on the direct implicit-GEMM kernels with two-level summation, "
                                     "dgrad / wgrad on Winograd F(6x6,3x3) - at 256x256 the parameter gradients a median 9.5e-4 "
                                     "from float64 (PyTorch's own fp32: 7.6e-4; the all-Winograd default: 3e-3 on this network's "
                                     "ill-conditioned gradients); = MMH_WINOGRAD=bwd")),
    ("--fp32_exact_fwd", dict(type=str, default="direct", choices=["direct", "wino2"],
                              help="with --fp32_exact_grads only: the forward of the eligible 3x3 stride-1 convs - direct: the "
                                   "implicit-GEMM kernel with two-level summation; wino2: Winograd F(2x2,3x3) with the same "
                                   "two-level summation in its 16 GEMMs (= MMH_WINOGRAD=bwd_f2); no effect on the 16-bit opt levels")),
    ("--graph_step", dict(action="store_true",
                          help="single process: capture one optimize_parameters() - forward, three backward passes, three Adam "
                               "steps - into a hipGraph after a few eager iterations and replay it (Adam step count / lr, dropout "
                               "salt and image-pool decisions live behind device pointers); = MMH_GRAPH_STEP=1")),
    ("--device_png", dict(action="store_true",
                          help="with --dataroot: the loader uploads the PNG files' bytes and the device inflates and unfilters "
                               "them (mmh_png_decode_batch); files that are not 8-bit RGB non-interlaced go through PIL; "
                               "= MMH_DEVICE_PNG=1")),
    ("--resize_inputs", dict(type=int, default=0,
                             help="with --dataroot: feed the networks N x N images whatever size the files hold (0 = the "
                                  "files' size); bilinear with half-pixel centres inside the device's decode pass, joints "
                                  "scaled with it, sigma unchanged; N a multiple of 4")),
    ("--resident_dataset", dict(action="store_true",
                                help="with --dataroot: keep the decoded images of this rank's batches in device memory (the "
                                     "loader's order never changes between epochs); the first epoch reads the files as usual and "
                                     "fills the store, every later batch is one kernel reading it by index "
                                     "(mmh_decode_inputs_indexed) - no file read, no PNG decode, no upload; "
                                     "= MMH_RESIDENT_DATASET=1")),
    ("--resident_gb", dict(type=float, default=64.0,
                           help="with --resident_dataset: the most device memory the store may take, in GB (10^9 bytes).  The "
                                "default is a policy choice - under a quarter of a 288 GB card - not a measured number; a "
                                "dataset over it (or over the free memory) leaves the loader on the file path, whole: there "
                                "is no partial store")),
    ("--pairing", dict(type=str, default="random", choices=["random", "curriculum", "nearest"],
                       help="with --dataroot: how a target gets its source - random: the reference's shuffle; curriculum: the "
                            "same random pairs, fed from the smallest pose distance (nearest_neighbor_search.py:68-83) to the "
                            "largest, every epoch; nearest: the source whose 3D pose is closest to the target's")),
    ("--match_pool", dict(type=str, default="self", choices=["self", "train"],
                          help="with --pairing nearest: where the sources come from - self: the loader's own targets, the target "
                               "itself excluded; train: the training share of the same --dataroot, for a generation split")),
    ("--depth_source", dict(type=str, default="files", choices=["files", "joints"],
                            help="with --dataroot: where the depth conditions D1 / D2 come from - files: the depth PNG beside "
                                 "every colour PNG; joints: rendered on the device from the 3D joints C1 / C2 right after the "
                                 "decode pass (mmh_render_pose_depth: 20 bones as capsules with a depth test) - no depth file "
                                 "is opened, and --resident_dataset holds one slot per colour file")),
    ("--render_radius", dict(type=float, default=5.0,
                             help="with --depth_source joints: half-width of a bone in pixels of the grid the networks see; "
                                  "like sigma it is not scaled by --resize_inputs or --augment_geom")),
    ("--render_bg", dict(type=float, default=255.0,
                         help="with --depth_source joints: the depth of a pixel no bone covers, in C1 / C2's units "
                              "(depth / 700 * 255); 255 maps to +1")),
]
_TRAIN = [
    ("--display_freq", dict(type=int, default=100)),
    ("--display_single_pane_ncols", dict(type=int, default=0)),
    ("--update_html_freq", dict(type=int, default=1000)),
    ("--print_freq", dict(type=int, default=100)),
    ("--save_latest_freq", dict(type=int, default=5000)),
    ("--save_epoch_freq", dict(type=int, default=1)),
    ("--continue_train", dict(action="store_true")),
    ("--epoch_count", dict(type=int, default=1)),
    ("--phase", dict(type=str, default="train")),
    ("--which_epoch", dict(type=str, default="latest")),
    ("--niter", dict(type=int, default=500)),
    ("--niter_decay", dict(type=int, default=200)),
    ("--beta1", dict(type=float, default=0.5)),
    ("--lr", dict(type=float, default=0.0002)),
    ("--no_lsgan", dict(action="store_true")),
    ("--lambda_A", dict(type=float, default=10.0)),
    ("--lambda_B", dict(type=float, default=10.0)),
    ("--lambda_GAN", dict(type=float, default=5.0)),
    ("--pool_size", dict(type=int, default=50)),
    ("--no_html", dict(action="store_true")),
    ("--lr_policy", dict(type=str, default="lambda")),
    ("--lr_decay_iters", dict(type=int, default=50)),
    ("--L1_type", dict(type=str, default="l1_plus_perL1")),
    ("--perceptual_layers", dict(type=int, default=3)),
    ("--percep_is_l1", dict(type=int, default=1)),
    ("--no_dropout_D", dict(action="store_true")),
    ("--DG_ratio", dict(type=int, default=1)),
    ("--augment_geom", dict(action="store_true",
                            help="with --dataroot: a random rotation, scale, shift (and flip) per image and epoch, sampled "
                                 "inside the device's decode pass (mmh_decode_inputs_affine; bilinear, edge replicate); joints "
                                 "transformed with the pixels, sigma unchanged")),
    ("--aug_rotate", dict(type=float, default=15.0, help="with --augment_geom: degrees, theta ~ U(-r, r)")),
    ("--aug_scale", dict(type=float, default=0.1, help="with --augment_geom: s ~ U(1 - a, 1 + a), 0 <= a < 1")),
    ("--aug_shift", dict(type=float, default=0.05, help="with --augment_geom: shift ~ U(-f, f) of the image size, per axis")),
    ("--aug_flip", dict(type=float, default=0.0,
                        help="with --augment_geom: probability of a horizontal flip (0 by default: a mirrored hand is the other hand)")),
    ("--aug_pair", dict(type=str, default="shared", choices=["shared", "independent"],
                        help="with --augment_geom: shared - source and target of a pair take one draw (the pair keeps the "
                             "relation it has in the data, background included); independent - each draws its own")),
    ("--aug_seed", dict(type=int, default=0, help="with --augment_geom: seed of the draws (with the epoch number)")),
]
_TEST = [
    ("--ntest", dict(type=int, default=float("inf"))),
    ("--results_dir", dict(type=str, default="./results/")),
    ("--aspect_ratio", dict(type=float, default=1.0)),
    ("--phase", dict(type=str, default="test")),
    ("--which_epoch", dict(type=str, default="latest")),
    ("--how_many", dict(type=int, default=200)),
]


def check_exact_fwd(opt):
    """--fp32_exact_fwd chooses the forward of the gradient-exact hybrid: without --fp32_exact_grads there is none"""
    if getattr(opt, "fp32_exact_fwd", "direct") not in ("direct", "wino2"):
        raise ValueError(f"--fp32_exact_fwd {opt.fp32_exact_fwd!r}: expected direct | wino2")
    if getattr(opt, "fp32_exact_fwd", "direct") != "direct" and not getattr(opt, "fp32_exact_grads", False):
        raise ValueError("--fp32_exact_fwd wino2 needs --fp32_exact_grads (it selects that hybrid's forward kernels)")
    return opt


def check_resize_inputs(opt):
    """--resize_inputs N: 0 = off, else the square target of the device's decode pass - a multiple of 4, as the networks'
    two stride-2 stages need it.  Returns N."""
    n = getattr(opt, "resize_inputs", 0) or 0
    if isinstance(n, bool) or not isinstance(n, int) or n < 0 or n % 4 != 0:
        raise ValueError(f"--resize_inputs {n!r}: expected 0 (off) or a positive multiple of 4")
    return n


DEPTH_SOURCES = ("files", "joints")


def check_depth_source(opt, need_dataroot=True):
    """--depth_source with --render_radius / --render_bg, validated; absent attributes are the defaults.  Returns None for
    `files`, else (radius, bg).  need_dataroot=False: for a consumer of batches (MMHandModel), which has no loader to ask."""
    src = getattr(opt, "depth_source", None) or "files"
    if src not in DEPTH_SOURCES:
        raise ValueError(f"--depth_source {src!r}: expected one of {' | '.join(DEPTH_SOURCES)}")

    def num(name, default):
        v = getattr(opt, name, default)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"--{name} {v!r}: a finite number expected")
        return float(v)

    radius, bg = num("render_radius", 5.0), num("render_bg", 255.0)
    if radius < 0.0:
        raise ValueError(f"--render_radius {radius!r}: expected pixels, >= 0")
    if src == "files":
        return None
    if need_dataroot and not getattr(opt, "dataroot", None):
        raise ValueError("--depth_source joints works with --dataroot only (the synthetic loader has no joints' depth)")
    return radius, bg


AUG_PAIRS = ("shared", "independent")


def check_augment(opt):
    """--augment_geom and its ranges, validated; absent attributes are the defaults.  Returns None when the flag is off, else
    (rotate, scale, shift, flip, pair, seed)."""
    if not getattr(opt, "augment_geom", False):
        return None

    def num(name, default):
        v = getattr(opt, name, default)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"--{name} {v!r}: a finite number expected")
        return float(v)

    rotate, scale, shift, flip = num("aug_rotate", 15.0), num("aug_scale", 0.1), num("aug_shift", 0.05), num("aug_flip", 0.0)
    if not 0.0 <= rotate <= 180.0:
        raise ValueError(f"--aug_rotate {rotate!r}: expected degrees in [0, 180]")
    if not 0.0 <= scale < 1.0:
        raise ValueError(f"--aug_scale {scale!r}: expected 0 <= a < 1 (s ~ U(1 - a, 1 + a) must stay positive)")
    if not 0.0 <= shift <= 1.0:
        raise ValueError(f"--aug_shift {shift!r}: expected a fraction of the image size in [0, 1]")
    if not 0.0 <= flip <= 1.0:
        raise ValueError(f"--aug_flip {flip!r}: expected a probability in [0, 1]")
    pair = getattr(opt, "aug_pair", None) or "shared"
    if pair not in AUG_PAIRS:
        raise ValueError(f"--aug_pair {pair!r}: expected one of {' | '.join(AUG_PAIRS)}")
    seed = getattr(opt, "aug_seed", 0)
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
        raise ValueError(f"--aug_seed {seed!r}: a non-negative integer expected")
    if not getattr(opt, "dataroot", None):
        raise ValueError("--augment_geom works with --dataroot only (the synthetic loader has no images to transform)")
    return rotate, scale, shift, flip, pair, seed


def check_augment_color(opt):
    """--augment_color of train_hpe and its ranges, validated; absent attributes are the defaults.  Returns None when the flag
    is off, else (saturation, hue, gain, gamma, seed): s ~ U(1 - a, 1 + a) clipped at 0, h ~ U(-d, d) degrees,
    gain ~ U(1 - g, 1 + g) per channel, gamma = exp(U(-q, q))."""
    if not getattr(opt, "augment_color", False):
        return None

    def num(name, default):
        v = getattr(opt, name, default)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"--{name} {v!r}: a finite number expected")
        return float(v)

    sat, hue, gain, gamma = num("aug_saturation", 0.3), num("aug_hue", 10.0), num("aug_gain", 0.1), num("aug_gamma", 0.2)
    if sat < 0.0:
        raise ValueError(f"--aug_saturation {sat!r}: expected a >= 0 (s ~ U(1 - a, 1 + a), clipped at 0)")
    if not 0.0 <= hue <= 180.0:
        raise ValueError(f"--aug_hue {hue!r}: expected degrees in [0, 180]")
    if not 0.0 <= gain < 1.0:
        raise ValueError(f"--aug_gain {gain!r}: expected 0 <= g < 1 (a gain ~ U(1 - g, 1 + g) must stay positive)")
    if not 0.0 <= gamma <= 4.0:
        raise ValueError(f"--aug_gamma {gamma!r}: expected 0 <= q <= 4 (gamma = exp(U(-q, q)))")
    seed = getattr(opt, "aug_seed", 0)
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
        raise ValueError(f"--aug_seed {seed!r}: a non-negative integer expected")
    return sat, hue, gain, gamma, seed


class BaseOptions:
    isTrain = None
    _extra = []

    def __init__(self):
        self.parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        self.initialized = False

    def initialize(self):
        for flag, kw in _BASE + self._extra:
            self.parser.add_argument(flag, **kw)
        self.initialized = True

    def parse(self, args=None, init_dist=True, save=True):
        if not self.initialized:
            self.initialize()
        opt = self.parser.parse_args(args)
        try:
            check_exact_fwd(opt)
        except ValueError as e:
            self.parser.error(str(e))
        check_resize_inputs(opt)        # a ValueError, as for a namespace built in code (MMHandModel checks those)
        check_augment(opt)              # likewise (data.HandFolderLoader checks those)
        check_depth_source(opt)         # likewise
        opt.isTrain = self.isTrain
        import torch
        if opt.distributed:
            opt.local_rank = int(os.environ.get("LOCAL_RANK", opt.local_rank))
            opt.gpu = opt.local_rank
            if torch.cuda.is_available():
                torch.cuda.set_device(opt.gpu)
            if init_dist and not torch.distributed.is_initialized():
                backend = "nccl" if torch.cuda.is_available() else "gloo"
                torch.distributed.init_process_group(backend=backend, init_method="env://")
            opt.world_size = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
            if opt.batchSize is not None:
                opt.batchSize = opt.batchSize // opt.world_size   # base_options.py:178
            opt.gpu_ids = [opt.local_rank]
        else:
            opt.gpu_ids = [int(s) for s in str(opt.gpu_ids).split(",") if int(s) >= 0]
            opt.gpu = opt.gpu_ids[0] if opt.gpu_ids else -1
            if opt.gpu_ids and torch.cuda.is_available():
                torch.cuda.set_device(opt.gpu_ids[0])
            opt.world_size = 1
        self.opt = opt
        if save:
            self._dump(opt)
        return opt

    @staticmethod
    def _dump(opt):
        lines = ["------------ Options -------------"]
        lines += ["%s: %s" % (k, v) for k, v in sorted(vars(opt).items())]
        lines += ["-------------- End ----------------"]
        if opt.local_rank == 0:
            print("\n".join(lines))
            expr_dir = os.path.join(opt.checkpoints_dir, opt.name)
            os.makedirs(expr_dir, exist_ok=True)
            with open(os.path.join(expr_dir, "opt.txt"), "wt") as f:
                f.write("\n".join(lines) + "\n")


class TrainOptions(BaseOptions):
    isTrain = True
    _extra = _TRAIN


class TestOptions(BaseOptions):
    isTrain = False
    _extra = _TEST


def default_train_opt(**overrides):
    """Programmatic TrainOptions namespace (defaults of the tables above) for bench/tests.  Never
    touches the current CUDA device or the process group: the caller owns both.  Unlike the command
    line it opts in to --vgg_random_init (bench and tests have no pretrained VGG file)."""
    o = TrainOptions()
    o.initialize()
    opt = o.parser.parse_args([])
    opt.isTrain = True
    lr = int(overrides.get("local_rank", 0))
    opt.gpu_ids = [lr]
    opt.gpu = lr
    opt.world_size = 1
    opt.vgg_random_init = True
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt
