"""Detection demo: run the detector of a config on image files and save the annotated pictures; the command line of ref:demo.py.

    python demo.py --input a.jpg b.jpg --output out_dir --opts MODEL.WEIGHTS w.pth

--heatmap objectness | attention | <buffer>[:<channel>] (p4, pos3:17, ...) lays that heat map of the detection pass under the boxes
(--heatmap-alpha, --heatmap-colormap jet | gray).  --track follows the detections from frame to frame (ids that persist, boxes coloured and
labelled by them) over a video, or over several --input images taken as a sequence in the given order, and prints the number of tracks
started.  --track-motion belt (with --track) is for a scene that moves as one, a conveyor belt: the frame's shift is voted from the boxes
and the tracks are moved by it before they are matched (--belt-radius: the largest shift per frame in pixels, --belt-bin: pixels per
histogram bin), and the mean shift per frame is printed beside the tracks started.  Images are decoded with Pillow and drawn on the device.  Video (--video-input, --webcam) needs OpenCV to decode and to show frames;
this package neither ships nor requires it, and the two flags say so when it is missing.
--support-json ANN.json --support-root DIR [--shots N] enrols every category of a COCO json from its annotated images (under DIR) before
the first frame: support crops and prototypes are computed on the device, in place of a support_feature.pkl.  With more than one
category every one of them is detected (N-way).
--rectify-quad x0 y0 x1 y1 x2 y2 x3 y3 is for a camera that looks at the belt obliquely: the four points of the camera frame where the
belt plane's corners top-left, top-right, bottom-right, bottom-left lie.  Every frame is warped into that plane on the device before
anything else looks at it, and the outputs are written rectified, at --rectify-size W H (default: the input frame's size; there is no
anti-aliasing, so keep it near the belt region's resolution in the camera frame)."""
import argparse
import glob
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CONFIG = os.path.join(HERE, "configs", "fsod", "finetune_vovnet.yaml")


def get_parser():
    parser = argparse.ArgumentParser(description="Draw the few-shot detector's boxes, class names and scores on images (on the GPU).")
    parser.add_argument("--config-file", default=DEFAULT_CONFIG, metavar="FILE", help="the model's yaml config (default: %(default)s)")
    parser.add_argument("--input", nargs="+", metavar="IMAGE", help="image files, or one quoted glob pattern")
    parser.add_argument("--output", metavar="PATH", help="where the pictures go: a directory, or a file name when there is one input")
    parser.add_argument("--confidence-threshold", type=float, default=0.9, metavar="T", help="detections scoring below T are not drawn (default: %(default)s)")
    parser.add_argument("--heatmap", metavar="KIND", help="lay a heat map of the pass under the boxes: objectness, attention, or a level buffer "
                        "with an optional channel such as p4 or pos3:17")
    parser.add_argument("--heatmap-alpha", type=int, default=128, metavar="A", help="the heat map's opacity, 0 .. 255 (default: %(default)s)")
    parser.add_argument("--heatmap-colormap", default="jet", choices=("jet", "gray"), help="the heat map's colour table (default: %(default)s)")
    parser.add_argument("--track", action="store_true", help="follow the detections across the frames: ids that persist, colours and labels by id; "
                        "needs --video-input, --webcam or several --input frames (a sequence in the given order); prints the tracks started")
    parser.add_argument("--track-motion", choices=("belt",), default=None, help="with --track: 'belt' votes the one shift the whole frame shares "
                        "and moves the tracks by it before matching (a conveyor belt); prints the mean shift per frame as well")
    parser.add_argument("--belt-radius", type=int, default=None, metavar="PX", help="with --track-motion belt: the largest shift per frame and axis "
                        "in pixels (default: 128; at most 64 bins of --belt-bin)")
    parser.add_argument("--belt-bin", type=int, default=None, choices=(1, 2, 4, 8, 16), metavar="PX", help="with --track-motion belt: pixels per "
                        "histogram bin, 1, 2, 4, 8 or 16 (default: 2)")
    parser.add_argument("--rectify-quad", type=float, nargs=8, default=None, metavar="PX", help="x0 y0 x1 y1 x2 y2 x3 y3: where the belt plane's "
                        "corners (top-left, top-right, bottom-right, bottom-left) lie in the camera frame; every frame is warped into that "
                        "plane on the device first and the outputs are written rectified")
    parser.add_argument("--rectify-size", type=int, nargs=2, default=None, metavar=("W", "H"), help="with --rectify-quad: the size of the "
                        "rectified frame (default: the input frame's size)")
    parser.add_argument("--support-json", metavar="ANN.json", help="enrol every category of this COCO annotation file as a support class before "
                        "the first frame (instead of support_feature.pkl); needs --support-root")
    parser.add_argument("--support-root", metavar="DIR", help="the directory of the images --support-json names")
    parser.add_argument("--shots", type=int, default=None, metavar="N", help="with --support-json: the first N annotations of each category (default: all)")
    parser.add_argument("--video-input", metavar="VIDEO", help="annotate a video file instead (needs OpenCV)")
    parser.add_argument("--webcam", action="store_true", help="annotate the first camera's frames instead (needs OpenCV)")
    parser.add_argument("--opts", nargs=argparse.REMAINDER, default=[], metavar="KEY VALUE", help="config overrides, e.g. MODEL.WEIGHTS model.pth; must come last")
    return parser


def setup_cfg(args):
    """The frozen config of the run.  The second stage's score threshold is the one knob this detector reads at test time."""
    from fewx.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(list(args.opts))
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = float(args.confidence_threshold)
    cfg.freeze()
    return cfg


def enrol_support(model, args, log):
    """--support-json: every category of the annotation file becomes a support class of the model."""
    from fewx.data.datasets.register_coco import load_coco_json
    from fewx.data.support import enrol_from_records
    shots = enrol_from_records(model, load_coco_json(args.support_json, args.support_root, extra_annotation_keys=["id"]), shot=args.shots)
    if not shots:
        sys.exit(f"demo.py: {args.support_json} holds no annotation to enrol")
    if len(shots) > 1:
        model.support_classes = "all"
    log.info("enrolled %s from %s", ", ".join(f"class {c}: {n} shots" for c, n in shots.items()), args.support_json)


def make_rectifier(args, cv2=None):
    """--rectify-quad / --rectify-size as an orehip.Rectifier, or None.  Without a size it is the first input frame's."""
    if args.rectify_quad is None:
        return None
    import orehip
    if args.rectify_size is not None:
        w, h = args.rectify_size
    elif args.input:
        from PIL import Image
        with Image.open(input_paths(args.input)[0]) as im:
            w, h = im.size
    else:
        capture = cv2.VideoCapture(0 if args.webcam else args.video_input)
        w, h = int(capture.get(cv2.CAP_PROP_FRAME_WIDTH)), int(capture.get(cv2.CAP_PROP_FRAME_HEIGHT))
        capture.release()
    try:
        return orehip.Rectifier(quad=[args.rectify_quad[k:k + 2] for k in range(0, 8, 2)], out_hw=(int(h), int(w)))
    except ValueError as err:
        sys.exit(f"demo.py: --rectify-quad / --rectify-size: {err}")


def input_paths(patterns):
    """The image paths of --input: several names are taken as they are, a single one may be a glob pattern."""
    if len(patterns) > 1:
        return list(patterns)
    found = sorted(glob.glob(os.path.expanduser(patterns[0])))
    if not found:
        sys.exit(f"demo.py: no file matches {patterns[0]!r}")
    return found


def output_path(output, image_path, n_inputs):
    if os.path.isdir(output):
        return os.path.join(output, os.path.basename(image_path))
    if n_inputs > 1:
        sys.exit(f"demo.py: {n_inputs} inputs need a directory as --output, and {output!r} is not one")
    return output


def run_images(demo, args, log):
    from detectron2.data.detection_utils import read_image
    paths = input_paths(args.input)
    for path in paths:
        target = output_path(args.output, path, len(paths))
        predictions, picture = demo.run_on_image(read_image(path, format="BGR"))
        picture.save(target)
        log.info("%s: %d detections -> %s", path, len(predictions["instances"]), target)


def run_sequence(demo, args, log):
    """--track over image files: the inputs are the frames of one sequence, in the order given."""
    from PIL import Image
    from detectron2.data.detection_utils import read_image
    paths = input_paths(args.input)
    if len(paths) < 2:
        sys.exit("demo.py: --track needs a sequence: --video-input, --webcam or at least two --input frames")
    targets = [output_path(args.output, path, len(paths)) for path in paths]
    for path, target, frame in zip(paths, targets, demo.run_on_video(read_image(path, format="BGR") for path in paths)):
        Image.fromarray(frame[:, :, ::-1].copy()).save(target)
        log.info("%s -> %s", path, target)


def run_video(demo, args, cv2):
    capture = cv2.VideoCapture(0 if args.webcam else args.video_input)
    writer = None
    try:
        for frame in demo.run_on_video(capture):
            if args.output:
                if writer is None:
                    rate = capture.get(cv2.CAP_PROP_FPS) or 30.0
                    writer = cv2.VideoWriter(args.output, cv2.VideoWriter_fourcc(*"mp4v"), float(rate), (frame.shape[1], frame.shape[0]), True)
                writer.write(frame)
            else:
                cv2.imshow("detections", frame)
                if cv2.waitKey(1) == 27:                      # Esc ends the show
                    break
    finally:
        capture.release()
        if writer is not None:
            writer.release()


def main(argv=None):
    args = get_parser().parse_args(argv)
    video = args.webcam or bool(args.video_input)
    cv2 = None
    if video:
        if args.input:
            sys.exit("demo.py: --input and a video source exclude each other")
        try:
            import cv2
        except ImportError:
            flag = "--webcam" if args.webcam else "--video-input"
            sys.exit(f"demo.py: {flag} needs OpenCV (the cv2 module) to decode and show video, and it is not installed. "
                     "Annotate image files with --input, or hand your own frames to predictor.VisualizationDemo.run_on_video.")
    elif not args.input:
        sys.exit("demo.py: nothing to do; name images with --input (or a video with --video-input / --webcam)")
    elif args.track and len(args.input) < 2 and not any(ch in args.input[0] for ch in "*?["):
        sys.exit("demo.py: --track needs a sequence: --video-input, --webcam or at least two --input frames")
    elif not args.output:
        sys.exit("demo.py: --input needs --output: pictures are written to files, there is no window to show them in")
    if args.track_motion and not args.track:
        sys.exit("demo.py: --track-motion goes with --track")
    if (args.belt_radius is not None or args.belt_bin is not None) and args.track_motion != "belt":
        sys.exit("demo.py: --belt-radius and --belt-bin go with --track-motion belt")
    belt = {k: v for k, v in (("radius", args.belt_radius), ("bin", args.belt_bin)) if v is not None}
    if args.track_motion == "belt":
        bin_, radius = belt.get("bin", 2), belt.get("radius", 128)
        if radius < 1 or -(-radius // bin_) > 64:
            sys.exit(f"demo.py: --belt-radius {radius} at --belt-bin {bin_} is outside 1 .. {64 * bin_} (64 bins a side); use a larger bin")
    if args.rectify_size is not None and args.rectify_quad is None:
        sys.exit("demo.py: --rectify-size goes with --rectify-quad")
    if bool(args.support_json) != bool(args.support_root) or (args.shots is not None and not args.support_json):
        sys.exit("demo.py: --support-json and --support-root go together (and --shots with them)")
    if args.shots is not None and args.shots < 1:
        sys.exit("demo.py: --shots must be at least 1")

    from detectron2.utils.logger import setup_logger
    from predictor import VisualizationDemo, heatmap_args
    log = setup_logger()
    heatmap = {"kind": args.heatmap, "alpha": args.heatmap_alpha, "lut": args.heatmap_colormap} if args.heatmap else None
    try:
        heatmap = heatmap_args(heatmap, "--heatmap")          # the flags alone, before anything is built
    except ValueError as err:
        sys.exit(f"demo.py: {err}")
    rectify = make_rectifier(args, cv2)
    if args.track_motion == "belt":
        demo = VisualizationDemo(setup_cfg(args), heatmap=heatmap, track="belt", belt=belt, rectify=rectify)
    else:
        demo = VisualizationDemo(setup_cfg(args), heatmap=heatmap, track=args.track, rectify=rectify)
    if args.support_json:
        enrol_support(demo.predictor.model, args, log)
    if video:
        run_video(demo, args, cv2)
    elif args.track:
        run_sequence(demo, args, log)
    else:
        run_images(demo, args, log)
    if args.track:
        stats = demo.track_stats()
        if args.track_motion == "belt":
            k = max(stats["frames"], 1)
            print(f"tracks started: {stats['started']}; mean shift per frame: ({stats.get('travel', (0, 0))[0] / k:.1f}, {stats.get('travel', (0, 0))[1] / k:.1f}) px "
                  f"over {stats['frames']} frames, {stats.get('coasted', 0)} coasted")
        else:
            print(f"tracks started: {stats['started']}")


if __name__ == "__main__":
    main()
