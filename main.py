#!/usr/bin/env python3
"""Command-line entry, same flags as the reference's ``main.py:11-109``:

    python main.py -p infer -m mpp -c mpp_hrcM [-d DATASET] [-o] [--figures] [--birth-map] [--birth-complete] [--descent]
                   [--restarts R [--tempering [RATIO]] [--recombine]]
    python main.py -p detect -m mpp -c mpp_hrcM --images PATH [PATH ...] --out DIR [--gsd G] [--figures] [--birth-map] [--birth-complete] [--descent]

``-m mpp`` runs the MI355X sampler; ``-m posnet`` / ``-m shapenet`` with ``-p infer`` write the score-map
hand-off pickles the reference's MPP stage reads (``NNNN_results.pkl``) and the CNN-only baseline's detections (DOTA hbb /
obb files), ``-p eval`` scores those.  ``-p train -m mpp`` learns the
energy weights (manual / ordering / integral criterion) and calibrates; ``-p train -m posnet|shapenet`` trains the two
U-Nets on one GPU (batches built and losses computed by HIP kernels, ``unet_training.train_unet``; with the shipped configs
that includes histogram matching, the whole ``strong`` augmentation recipe (shadow, fog, CLAHE, downscale and blur built as
HIP kernels too) and, for PosNet, the error-density resampling of ``data_loader.error_update_interval``,
whose maps land in ``<dataset base>/error_maps/<dataset>/train/<model_name>/``).  With ``torchrun --nproc-per-node N`` the images of the dataset are
dealt to N GPUs (one gather of the results at the end; RCCL).

``-p detect`` runs the detector (U-Nets + sampler) on any image files, no dataset or annotation needed, and writes
``<stem>_detections.csv`` / ``<stem>_results.pkl`` (and, with ``--figures``, ``<stem>_detection.png``) in the pixels of each
file (``detect.py``).  ``--figures`` with ``-p infer`` writes the reference's two pictures per image; ``-p data_preview -m mpp``
the annotation over each ``val`` image.

``-p translate_dota -c <config>`` / ``-p translate_cowc -c <config>`` (no ``-m``) turn a raw DOTA or COWC download into the
dataset layout all of the above read (``dataset_translation``; the rescale to the target GSD is a HIP kernel; example configs
in ``model_configs/translation/``).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _restarts(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError(f"{text}: at least 1")
    return v


def _ratio(text):
    v = float(text)
    if not (v >= 1.0) or v == float("inf"):
        raise argparse.ArgumentTypeError(f"{text}: a finite ratio of at least 1")
    return v


def _radius(text):
    v = int(text)
    if not 1 <= v <= 7:
        raise argparse.ArgumentTypeError(f"{text}: a radius of 1..7 pixels")
    return v


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-m", "--model", help="model to use")
    parser.add_argument("-d", "--dataset", help="dataset to use, defaults to the one specified in config")
    parser.add_argument("-p", "--procedure", help="procedure to execute")
    parser.add_argument("-c", "--config", help="model config file, or the name of a stored model")
    parser.add_argument("-o", "--overwrite", action="store_true", help="overwrite existing results")
    parser.add_argument("-r", "--resume", action="store_true", help="(training) resume from checkpoint")
    parser.add_argument("--spec-waves", type=int, default=None,
                        help="speculative waves per chain (1,2,4,8,16); default: chosen per launch from the number of tiles and the "
                             "LDS footprint of a chain (sampler.choose_spec_waves)")
    parser.add_argument("--unet", action="store_true", help="compute the score maps with the U-Nets on the GPU "
                                                            "instead of reading NNNN_results.pkl")
    parser.add_argument("--unet-max-pixels", type=int, default=None,
                        help="at most this many (padded) pixels per U-Net forward: larger images are walked in crops whose "
                             "maps are stitched exactly (unet.chunk_plan); default: the whole image at once, in crops only "
                             "if that runs out of device memory")
    parser.add_argument("--restarts", type=_restarts, default=None,
                        help="(-m mpp, infer / infereval) independent chains per tile, the lowest-energy one is kept; "
                             "overrides inference.restarts of the config (default 1)")
    parser.add_argument("--tempering", type=_ratio, nargs="?", const=True, default=None, metavar="RATIO",
                        help="(-m mpp, infer / infereval / detect) parallel tempering: the restarts of a tile anneal on a ladder of "
                             "temperatures, RATIO apart from rung to rung (default: the sampler's), and neighbouring rungs "
                             "exchange their schedules at intervals; needs --restarts or inference.restarts of at least 2; same "
                             "as inference.tempering in the config (whose 'every' it keeps); off by default")
    parser.add_argument("--recombine", action="store_true",
                        help="(-m mpp, infer / infereval / detect) recombine the restarts of a tile: every interaction cluster of "
                             "the returned configuration comes from the restart that spends the least energy there, instead of "
                             "the lowest-energy restart as a whole; needs --restarts or inference.restarts of at least 2; same as "
                             "inference.recombine in the config; off by default")
    parser.add_argument("--figures", action="store_true",
                        help="(-m mpp, infer / infereval / detect) write the result pictures composed on the GPU: NNNN_detection.png, "
                             "NNNN_gt.png (and NNNN_detection_map.png) beside NNNN_results.pkl; same as inference.figures in the config")
    parser.add_argument("--birth-map", action="store_true",
                        help="(-m mpp, infer / infereval / detect) per image the birth-energy map under its detections -- the energy "
                             "change of a new object at every pixel: NNNN_birth_energy.png, the key birth_summary of the pickle and "
                             "one log line; same as inference.birth_map in the config")
    parser.add_argument("--birth-complete", action="store_true",
                        help="(-m mpp, infer / infereval / detect) complete every image's detections from its birth-energy map: "
                             "births at the map's local minima, round after round, until no new object lowers the energy; the "
                             "results are those of the completed list, the pickle gains the key birth_complete and one line is "
                             "logged; same as inference.birth_complete in the config (whose max_rounds / min_gain it keeps)")
    parser.add_argument("--descent", action="store_true",
                        help="(-m mpp, infer / infereval / detect) local descent of every image's detections: rounds of greedy "
                             "deaths (objects whose removal lowers the energy) and of the births of --birth-complete, until a whole "
                             "round changes nothing; the results are those of the descended list, the pickle gains the key descent "
                             "and one line is logged; same as inference.descent in the config (whose parameters it keeps)")
    parser.add_argument("--relocate", type=_radius, nargs="?", const=True, default=None, metavar="RADIUS",
                        help="(-m mpp, infer / infereval / detect) relocation of every image's detections: every object moves to "
                             "the candidate of the score maps within RADIUS pixels (1..7, default: the config's, else 2) that "
                             "lowers the energy most, round after round, until none does; with --descent the two repeat while "
                             "something moves; the pickle gains the key relocate and one line is logged; same as "
                             "inference.relocate in the config (whose other parameters it keeps)")
    parser.add_argument("--images", nargs="+", default=None, metavar="PATH",
                        help="(-p detect) image files, or directories whose image files are taken in sorted order")
    parser.add_argument("--out", default=None, metavar="DIR", help="(-p detect) where the results go")
    parser.add_argument("--gsd", type=float, default=None,
                        help="(-p detect) ground sampling distance of the images in metres per pixel; finer than --model-gsd: the "
                             "images are reduced to it first (default: --model-gsd, no rescale)")
    parser.add_argument("--model-gsd", type=float, default=0.5, help="(-p detect) ground sampling distance the nets were trained at")
    parser.add_argument("--min-score", type=float, default=None, help="(-p detect) drop detections scored below this from the CSV")
    return parser


def apply_birth_complete(args, config):
    """--birth-complete turns inference.birth_complete on; parameters the config gives for it stay"""
    if args.birth_complete and args.procedure in ("infer", "infereval", "detect"):
        inference = config.setdefault("inference", {})
        if not isinstance(inference.get("birth_complete"), dict):
            inference["birth_complete"] = True
    return config


def apply_descent(args, config):
    """--descent turns inference.descent on; parameters the config gives for it stay"""
    if args.descent and args.procedure in ("infer", "infereval", "detect"):
        inference = config.setdefault("inference", {})
        if not isinstance(inference.get("descent"), dict):
            inference["descent"] = True
    return config


def apply_relocate(args, config):
    """--relocate turns inference.relocate on; --relocate RADIUS sets its radius; other parameters the config gives stay"""
    if args.relocate is not None and args.procedure in ("infer", "infereval", "detect"):
        inference = config.setdefault("inference", {})
        if args.relocate is not True:
            kept = inference["relocate"] if isinstance(inference.get("relocate"), dict) else {}
            inference["relocate"] = dict(kept, radius=args.relocate)
        elif not isinstance(inference.get("relocate"), dict):
            inference["relocate"] = True
    return config


def apply_recombine(args, config):
    """--recombine turns inference.recombine on"""
    if args.recombine and args.procedure in ("infer", "infereval", "detect"):
        config.setdefault("inference", {})["recombine"] = True
    return config


def apply_tempering(args, config):
    """--tempering turns inference.tempering on; --tempering RATIO sets its ratio; an interval the config gives stays"""
    if args.tempering is not None and args.procedure in ("infer", "infereval", "detect"):
        inference = config.setdefault("inference", {})
        if args.tempering is not True:
            kept = inference["tempering"] if isinstance(inference.get("tempering"), dict) else {}
            inference["tempering"] = dict(kept, ratio=args.tempering)
        elif not isinstance(inference.get("tempering"), dict):
            inference["tempering"] = True
    return config


def main():
    args = build_parser().parse_args()

    from mpp_cnn_rs_object_detection_amd.paths import get_model_base_path, resolve_model_config_path
    with open(resolve_model_config_path(args.config)) as f:
        config = json.load(f)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    overwrite_results = args.overwrite and args.procedure != "train"

    if args.procedure in ("translate_dota", "translate_cowc"):
        from mpp_cnn_rs_object_detection_amd import dataset_translation
        getattr(dataset_translation, args.procedure)(config, device=local_rank)
        print("done !")
        return

    if args.procedure == "train" and args.model in ("posnet", "shapenet"):
        from mpp_cnn_rs_object_detection_amd.unet_training import train_unet
        train_unet(config, args.model, dataset=args.dataset, device=local_rank, overwrite=args.overwrite, resume=args.resume)
        print("done !")
        return

    if args.procedure == "detect":
        if args.model != "mpp":
            raise ValueError("-p detect runs the MPP detector: -m mpp")
        if not args.images or not args.out:
            raise ValueError("-p detect needs --images PATH [PATH ...] and --out DIR")
        from mpp_cnn_rs_object_detection_amd import detect
        from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
        detect.resolve_scale(args.gsd, args.model_gsd)          # (a coarser picture is refused before anything is loaded)
        if args.restarts is not None:
            config.setdefault("inference", {})["restarts"] = args.restarts
        if args.birth_map:
            config.setdefault("inference", {})["birth_map"] = True
        apply_birth_complete(args, config)
        apply_descent(args, config)
        apply_relocate(args, config)
        apply_tempering(args, config)
        apply_recombine(args, config)
        model = MPPModel(config, phase="val", load=True, device=local_rank,
                         nets=load_nets(config, local_rank, args.unet_max_pixels), spec_waves=args.spec_waves)
        detect.detect_files(model, args.images, args.out, gsd=args.gsd, model_gsd=args.model_gsd, min_score=args.min_score,
                            figures=args.figures)
        print("done !")
        return

    if args.model == "mpp":
        from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
        if args.restarts is not None and args.procedure in ("infer", "infereval"):
            config.setdefault("inference", {})["restarts"] = args.restarts
        if args.figures:
            config.setdefault("inference", {})["figures"] = True
        if args.birth_map and args.procedure in ("infer", "infereval"):
            config.setdefault("inference", {})["birth_map"] = True
        apply_birth_complete(args, config)
        apply_descent(args, config)
        apply_relocate(args, config)
        apply_tempering(args, config)
        apply_recombine(args, config)
        nets = None
        if args.unet:
            nets = load_nets(config, local_rank, args.unet_max_pixels)
        # (data_preview only looks at the dataset: the stored model is loaded so that nothing is calibrated or trained for it)
        model = MPPModel(config, phase="train" if args.procedure == "train" else "val",
                         load=args.procedure != "train", dataset=args.dataset, device=local_rank,
                         nets=nets, spec_waves=args.spec_waves)
    elif args.model in ("posnet", "shapenet"):
        model = ScoreMapWriter(config, args.model, args.dataset, local_rank, args.unet_max_pixels)
    else:
        raise ValueError(f"model {args.model!r}: only mpp / posnet / shapenet inference is built")

    if args.procedure == "infer":
        print("infering on dataset")
        model.infer(subset="val", min_confidence=0.2, display_min_confidence=0.5, overwrite=overwrite_results)
    elif args.procedure == "infereval":
        model.infer(subset="val", min_confidence=0.2, display_min_confidence=0.5, overwrite=overwrite_results)
        model.eval()
    elif args.procedure == "eval":
        model.eval()
    elif args.procedure == "train":
        model.train()
    elif args.procedure == "data_preview":
        print("previewing data")
        model.data_preview()
    else:
        raise ValueError(args.procedure)
    print("done !")


def load_nets(mpp_config, device, max_forward_pixels=None):
    """PosNet + ShapeNet named by the MPP config, weights from <model_path>/{posnet,shapenet}/<name>/model.pt."""
    from mpp_cnn_rs_object_detection_amd import unet
    from mpp_cnn_rs_object_detection_amd.paths import get_model_base_path
    base = get_model_base_path()
    pos_dir = os.path.join(base, "posnet", mpp_config["dataset"]["position_model"])
    shp_dir = os.path.join(base, "shapenet", mpp_config["dataset"]["shape_model"])
    pos, shp = unet.PosNet(), unet.ShapeNet()
    if not unet.load_torch_model(pos, pos_dir) or not unet.load_torch_model(shp, shp_dir):
        raise FileNotFoundError(f"no model.pt / checkpoint_*.pt under {pos_dir} or {shp_dir}")
    return unet.ScoreMapNets(pos, shp, device=device, div_clf=unet.load_div_clf(pos_dir), max_forward_pixels=max_forward_pixels)


class ScoreMapWriter:
    """``-m posnet|shapenet -p infer|eval|infereval``: the reference's hand-off pickles (``pos_net_model.py:407-424`` /
    ``shape_net_model.py:353-381``) and the CNN-only baseline's detections.

    * posnet: candidates ``map > min_confidence``, distance NMS on the device, 12-px boxes in DOTA hbb files (ground truth:
      the same boxes at the annotated centres);
    * shapenet: centres from the PosNet named by ``config["inference"]["pos_model"]`` (``>=``, NMS; one forward gives both
      maps) or, without it, the annotated centres with score 1; a rectangle per centre from the argmax marks, in DOTA obb
      files.  ``eval`` runs ``dota_eval`` (hbb / obb) over the five IoU thresholds."""

    def __init__(self, config, kind, dataset, device, max_forward_pixels=None):
        from mpp_cnn_rs_object_detection_amd import unet
        from mpp_cnn_rs_object_detection_amd.paths import get_model_base_path
        self.kind, self.config, self.device = kind, config, device
        self.dataset = dataset or config["data_loader"]["dataset"]
        self.model_dir = os.path.join(get_model_base_path(), kind, config["model_name"])
        d = self.model_dir
        self.pos, self.shp = unet.PosNet(), unet.ShapeNet()
        if not unet.load_torch_model(self.pos if kind == "posnet" else self.shp, d):
            raise FileNotFoundError(f"no model.pt / checkpoint_*.pt under {d}")
        self.pos_model = config.get("inference", {}).get("pos_model") if kind == "shapenet" else None
        div_dir = d
        if self.pos_model:
            div_dir = os.path.join(get_model_base_path(), "posnet", self.pos_model)
            if not unet.load_torch_model(self.pos, div_dir):
                raise FileNotFoundError(f"no model.pt / checkpoint_*.pt under {div_dir} (inference.pos_model)")
        self.nets = unet.ScoreMapNets(self.pos, self.shp, device=device, div_clf=unet.load_div_clf(div_dir),
                                      max_forward_pixels=max_forward_pixels)

    def infer(self, subset, min_confidence=0.2, overwrite=True, **_):
        import logging
        import pickle
        import re
        import numpy as np
        from matplotlib import pyplot as plt
        from mpp_cnn_rs_object_detection_amd import cnn_detection as cd
        from mpp_cnn_rs_object_detection_amd import mappings
        from mpp_cnn_rs_object_detection_amd.dota_results import DOTAResultsTranslator
        from mpp_cnn_rs_object_detection_amd.paths import fetch_data_paths, get_inference_path
        from mpp_cnn_rs_object_detection_amd.shapes import rect_to_poly
        out_dir = get_inference_path(self.config["model_name"], self.dataset, subset)
        os.makedirs(out_dir, exist_ok=True)
        posnet = self.kind == "posnet"
        dota = DOTAResultsTranslator(self.dataset, subset, out_dir, "hbb" if posnet else "obb", all_classes=["vehicle"])
        if not posnet and not self.pos_model:
            logging.warning("no position inference model specified in config, falling back to using ground truth")
        paths = fetch_data_paths(self.dataset, subset)
        for pf, af in zip(paths["images"], paths["annotations"]):
            pid = int(re.match(r"([0-9]+).*.png", os.path.split(pf)[1]).group(1))
            out = os.path.join(out_dir, f"{pid:04}_results.pkl")
            if os.path.exists(out) and not overwrite:
                continue
            with open(af, "rb") as f:
                labels = pickle.load(f)
            gt_centers, gt_params = np.asarray(labels["centers"]), labels["parameters"]
            vehicle = lambda n: ["vehicle"] * n
            det, marks = self.nets.infer(plt.imread(pf)[:, :, :3])
            if posnet:
                det_np = det.cpu().numpy()
                cand = np.array(np.where(det_np > min_confidence)).T
                centers, scores, n_cand = cd.detect_centers(det, min_confidence, strict=True)
                assert n_cand == len(cand), (n_cand, len(cand))
                res = {"detection_map": det_np, "detection_type": "map", "detection": cand,
                       "detection_score": det_np[cand[:, 0], cand[:, 1]]}
                gt_poly = cd.box_polygons(cd.posnet_boxes(gt_centers))
                dota.add_gt(image_id=pid, polygons=gt_poly, difficulty=labels["difficult"], flip_coor=False,
                            categories=vehicle(len(gt_poly)))
                dota.add_detections(image_id=pid, scores=scores, bbox=cd.posnet_boxes(centers), flip_coor=False,
                                    class_names=vehicle(len(scores)))
            else:
                if self.pos_model:
                    centers, scores, _ = cd.detect_centers(det, min_confidence, strict=False)
                else:
                    centers, scores = gt_centers.astype(np.int64).reshape(-1, 2), np.ones(len(gt_centers))
                maps = mappings.default_mappings()
                params = cd.mark_params(marks, centers, maps)
                polys = cd.shapenet_polygons(centers, params)
                res = {"output": [m.permute(2, 0, 1).unsqueeze(0).cpu().numpy() for m in marks], "mappings": maps,
                       "detection": polys, "detection_type": "poly", "detection_center": centers, "detection_score": scores,
                       "detection_params": [tuple(p) for p in params], "pos_model": self.pos_model}
                gt_poly = np.array([rect_to_poly(c, short=p[0], long=p[1], angle=p[2]) for c, p in zip(gt_centers, gt_params)])
                dota.add_gt(image_id=pid, polygons=gt_poly, difficulty=labels["difficult"], categories=vehicle(len(gt_poly)))
                dota.add_detections(image_id=pid, scores=scores, polygons=polys, flip_coor=True, class_names=vehicle(len(scores)))
            with open(out, "wb") as f:
                pickle.dump(res, f)
        dota.save()

    def eval(self):
        from mpp_cnn_rs_object_detection_amd.dota_eval import dota_eval
        return dota_eval(model_dir=self.model_dir, dataset=self.dataset, subset="val",
                         det_type="hbb" if self.kind == "posnet" else "obb", device=self.device)


if __name__ == "__main__":
    main()
