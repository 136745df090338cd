"""Device-side alignment warp and paste-back: the detection-independent half of the reference's FaceRestoreHelper.

Mirror of facelib/utils/face_restoration_helper.py -- `align_warp_face` (:320-350), `get_inverse_affine` (:352-362),
`add_restored_face` (:364-369) and `paste_faces_to_input_image` (:372-499; square soft mask, optional parse-mask fusion) -- with the
frame, the crops, the masks and the upsampled canvas living in HBM and every OpenCV call replaced by a kernel of cf_paste.hip over the
face's bounding box (the reference filters the whole upsampled frame once per face).  Face DETECTION (RetinaFace, landmarks,
`cv2.estimateAffinePartial2D`) stays on the host as the north star says: the 2x3 alignment matrices are this class's input.

With a face upsampler (:388-392) every restored face is upsampled first -- all faces of the frame in ONE batched
`RealESRGANer.enhance_faces` call, or handed over already upsampled (`add_restored_faces(faces, upsampled=True)`) -- and pasted at
face_size * upscale with the rescaled inverse affine; with `draw_box` (:439-445, :502-509) the green border bands are blended in the
launch that also casts the frame to uint8 (cf_box_overlay_u8).

Differences from the reference, all stated in DESIGN.md: one device->host read-back per FRAME (the face areas that size the
feathering kernel, :433-441, and the box borders) instead of arrays crossing PCIe at every step; the parse-mask branch blends in
float32 where numpy promotes to float64 (the final image is truncated to uint8, so at most rare 1-LSB differences);
`inverse_affine_matrices` are not rescaled in place by a face-upsampled paste (the reference's are, which only shows when it pastes
twice); a face entirely outside the frame draws no box (the reference divides by its zero area).  The alpha channel of RGBA
backgrounds is not built.
"""
import math

import numpy as np
import torch

from .. import ops

MASK_COLORMAP = (0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 255, 0, 0, 0)   # :467


def invert_affine(m):
    """cv2.invertAffineTransform (double precision)."""
    m = np.asarray(m, dtype=np.float64).reshape(2, 3)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22, a12, a21 = m[1, 1] * d, m[0, 0] * d, -m[0, 1] * d, -m[1, 0] * d
    return np.array([[a11, a12, -a11 * m[0, 2] - a12 * m[1, 2]], [a21, a22, -a21 * m[0, 2] - a22 * m[1, 2]]], dtype=np.float64)


def gaussian_taps(ksize, sigma=0.0):
    """cv2.getGaussianKernel(ksize, sigma) as float32 taps: sigma <= 0 -> 0.3*((ksize-1)*0.5 - 1) + 0.8, with OpenCV's fixed tables
    for ksize <= 7 in that case."""
    small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and ksize in small:
        return np.asarray(small[ksize], dtype=np.float32)
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


class DeviceFaceHelper:
    """Per-frame state on the device: read_image -> align_warp_face(affines) -> [restore the crops] -> add_restored_faces ->
    paste_faces_to_input_image().  Method names follow FaceRestoreHelper; arrays are uint8 HWC BGR like cv2's."""

    def __init__(self, upscale_factor=1, face_size=512, device='cuda', use_parse=False, face_parse=None):
        self.upscale_factor = int(upscale_factor)
        self.face_size = (int(face_size), int(face_size))
        self.device = torch.device(device)
        self.use_parse = bool(use_parse)
        self.face_parse = face_parse              # a codeformer_amd.facelib.parsing ParseNet on `device` (needed when use_parse)
        self._ones = {}                           # face size -> ones((fh, fw)) (the square mask, :425)
        self._taps = {}
        self._partials = None
        self.clean_all()

    def clean_all(self):
        self.input_img = None
        self.affine_matrices = []
        self.inverse_affine_matrices = []
        self.cropped_faces = None
        self.restored_faces = None
        self.faces_upsampled = False

    def read_image(self, img):
        """img: uint8 (H,W,3) BGR numpy array or CUDA tensor (the decoded frame)."""
        t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError('read_image expects a uint8 HxWx3 image')
        self.input_img = t.to(self.device, non_blocking=True).contiguous()

    # ---- align_warp_face (:320-350) ------------------------------------------------------------------------------------------------
    def align_warp_face(self, affine_matrices):
        """affine_matrices: (n,2,3) frame -> face matrices (what estimateAffinePartial2D returned on the host).  All n crops are cut in
        ONE launch: cv2.warpAffine(input_img, M, face_size, borderMode=BORDER_CONSTANT, borderValue=(135, 133, 132)).
        Returns the uint8 (n, 512, 512, 3) crops on the device."""
        aff = np.asarray(affine_matrices, dtype=np.float64).reshape(-1, 2, 3)
        self.affine_matrices = [a.copy() for a in aff]
        n = aff.shape[0]
        fw, fh = self.face_size
        crops = torch.empty(n, fh, fw, 3, dtype=torch.uint8, device=self.device)
        if n:
            inv = np.stack([invert_affine(a) for a in aff]).reshape(n, 6)           # destination (face) pixel -> frame coordinate
            ops.warp_affine_u8(self.input_img, torch.from_numpy(inv).to(self.device), crops, border=(135, 133, 132))
        self.cropped_faces = crops
        return crops

    def get_inverse_affine(self):
        self.inverse_affine_matrices = [invert_affine(a) * self.upscale_factor for a in self.affine_matrices]   # :354-356
        return self.inverse_affine_matrices

    def add_restored_faces(self, restored, upsampled=False):
        """restored: uint8 (n,512,512,3) BGR CUDA tensor (cf_tensor_to_img_u8 output); upsampled=True: the faces already went through
        the face upsampler (uint8 (n,512*upscale,512*upscale,3)) and are pasted as the reference's face_upsampler branch does."""
        self.restored_faces = restored
        self.faces_upsampled = bool(upsampled)

    def upsample_faces(self, faces, face_upsampler):
        """face_upsampler.enhance(face, outscale=upscale)[0] for every face (:389): one batched call on the device when the upsampler
        has `enhance_faces` (RealESRGANer), else per face on the host with the reference's semantics."""
        u = self.upscale_factor
        if hasattr(face_upsampler, 'enhance_faces'):
            return face_upsampler.enhance_faces(faces, outscale=u)
        up = [np.ascontiguousarray(face_upsampler.enhance(f, outscale=u)[0]) for f in faces.cpu().numpy()]
        fw, fh = self.face_size
        if any(f.dtype != np.uint8 or f.shape != (fh * u, fw * u, 3) for f in up):
            raise ValueError(f'face_upsampler must return uint8 {(fh * u, fw * u, 3)} faces')
        return torch.from_numpy(np.stack(up)).to(self.device) if up else \
            torch.empty(0, fh * u, fw * u, 3, dtype=torch.uint8, device=self.device)

    # ---- parse mask (:455-481) -------------------------------------------------------------------------------------------------------
    def parse_soft_masks(self, restored):
        """ParseNet labels -> 0/255 map -> GaussianBlur(101, 11) twice -> 10-pixel border cleared -> / 255, per face, on the device."""
        if self.face_parse is None:
            raise RuntimeError('use_parse needs a ParseNet (face_parse=...)')
        x = ops.img_u8_to_tensor(restored)                                            # img2tensor(face/255.) + normalize(0.5, 0.5)
        labels = self.face_parse.parse_labels(x)                                      # (n,512,512) int64
        m = ops.label_lut(labels, MASK_COLORMAP)
        taps = self._taps_dev(101, 11.0)
        out = torch.empty_like(m)
        for i in range(m.shape[0]):
            out[i] = ops.gaussian_blur(ops.gaussian_blur(m[i], taps), taps)
        return ops.scale_clear_border_(out, 10, 1.0 / 255.0)

    def _taps_dev(self, ksize, sigma=0.0):
        key = (ksize, sigma)
        if key not in self._taps:
            self._taps[key] = torch.from_numpy(gaussian_taps(ksize, sigma)).to(self.device)
        return self._taps[key]

    # ---- paste_faces_to_input_image (:372-499) -----------------------------------------------------------------------------------------
    def _ones_dev(self, fw, fh):
        if (fw, fh) not in self._ones:
            self._ones[(fw, fh)] = torch.ones(fh, fw, dtype=torch.float32, device=self.device)
        return self._ones[(fw, fh)]

    @staticmethod
    def _region(inv_up, h_up, w_up, face_size):
        """Bounding box of the warped face square, grown by everything the masks can spread (erosions only shrink; the Gaussian
        spreads by its radius) and clipped to the canvas: outside it the soft mask is exactly 0."""
        fw, fh = face_size
        corners = np.array([[0, 0, 1], [fw, 0, 1], [0, fh, 1], [fw, fh, 1]], dtype=np.float64).T
        q = inv_up @ corners
        area = abs(inv_up[0, 0] * inv_up[1, 1] - inv_up[0, 1] * inv_up[1, 0]) * fw * fh
        margin = int(math.sqrt(area)) // 20 + 8
        x0, x1 = int(math.floor(q[0].min())) - margin, int(math.ceil(q[0].max())) + margin + 1
        y0, y1 = int(math.floor(q[1].min())) - margin, int(math.ceil(q[1].max())) + margin + 1
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w_up), min(y1, h_up)
        return (x0, y0, x1 - x0, y1 - y0) if (x1 > x0 and y1 > y0) else None

    @torch.no_grad()
    def paste_faces_to_input_image(self, upsample_img=None, return_tensor=False, face_upsampler=None, draw_box=False):
        """Returns the pasted uint8 (h_up, w_up, 3) BGR frame (numpy, or the CUDA tensor with return_tensor=True).
        upsample_img: optional uint8 background already at (h_up, w_up) (e.g. the Real-ESRGAN output).
        face_upsampler: upsample the restored faces first (:388-392; not needed when they were added with upsampled=True).
        draw_box: green border band around every face (:439-445, :502-509)."""
        h, w, _ = self.input_img.shape
        u = self.upscale_factor
        h_up, w_up = int(h * u), int(w * u)
        if upsample_img is None:
            canvas = ops.resize_linear_u8(self.input_img, h_up, w_up)                # cv2.resize(input_img, (w_up, h_up), INTER_LINEAR), :380
        else:
            bg = torch.from_numpy(np.ascontiguousarray(upsample_img)).to(self.device) if isinstance(upsample_img, np.ndarray) else upsample_img
            if tuple(bg.shape) != (h_up, w_up, 3):
                raise ValueError(f'upsample_img must be {(h_up, w_up, 3)} (resize it first), got {tuple(bg.shape)}')
            canvas = ops.resize_linear_u8(bg.contiguous(), h_up, w_up)
        faces = self.restored_faces
        n = 0 if faces is None else faces.shape[0]
        if not self.inverse_affine_matrices:
            self.get_inverse_affine()
        assert n == len(self.inverse_affine_matrices), 'length of restored_faces and affine_matrices are different.'
        upsampled = self.faces_upsampled or face_upsampler is not None
        fw, fh = self.face_size
        if upsampled:
            fw, fh = fw * u, fh * u                                                    # :392
            if n and not self.faces_upsampled:
                faces = self.upsample_faces(faces, face_upsampler)                     # :389, all faces of the frame in one call
            if n and tuple(faces.shape[1:]) != (fh, fw, 3):
                raise ValueError(f'upsampled faces must be {(fh, fw, 3)}, got {tuple(faces.shape[1:])}')
        parse = None
        if self.use_parse and n:
            # ParseNet sees the face at 512^2 (:459, cv2.resize INTER_LINEAR; at 2:1 that is (a+b+c+d+2)>>2).  The faces are stacked
            # as one tall image: at an integer ratio no output row reads a neighbouring face with a non-zero weight.
            small = faces
            if upsampled and u != 1:
                sw_, sh_ = self.face_size
                small = ops.f32_to_u8_trunc(ops.resize_linear_u8(faces.reshape(n * fh, fw, 3), n * sh_, sw_)).reshape(n, sh_, sw_, 3)
            parse = self.parse_soft_masks(small)
            if parse.shape[1:] != (fh, fw):
                parse = ops.resize_linear_f32(parse, fh, fw)                          # :482
        # phase 1 (all faces): warped square mask, first erosion, area partials -> ONE read-back per frame
        if self._partials is None or self._partials.shape[0] < max(n, 1):
            self._partials = torch.empty(max(n, 1), 64, dtype=torch.float64, device=self.device)
        ones = self._ones_dev(fw, fh)
        work = []
        for k in range(n):
            inv = self.inverse_affine_matrices[k].copy()                               # (the reference rescales its list in place)
            if upsampled:
                inv /= u                                                               # :390-391
                inv[:, 2] *= u
            else:
                inv[:, 2] += 0.5 * u if u > 1 else 0                                   # :393-398
            region = self._region(inv, h_up, w_up, (fw, fh))
            if region is None:
                work.append(None)
                self._partials[k].zero_()
                continue
            dst2src = invert_affine(inv)                                               # what cv2.warpAffine derives from its M
            inv_mask = ops.warp_affine_f32(ones, dst2src, region)                      # :428
            ero = ops.erode(inv_mask, int(2 * u))                                      # :430-431
            ops.sum_partials(ero, self._partials[k])                                   # :433
            work.append((region, dst2src, ero))
        areas = self._partials[:n].sum(dim=1).cpu().numpy() if n else []
        # phase 2: feathered mask + blend, face by face (the order matters where faces overlap)
        boxes = []
        for k in range(n):
            if work[k] is None:
                continue
            region, dst2src, ero = work[k]
            w_edge = int(float(areas[k]) ** 0.5) // 20                                 # :441
            center = ops.erode(ero, w_edge * 2)                                        # :443
            soft = ops.gaussian_blur(center, self._taps_dev(w_edge * 2 + 1), (region[0], region[1]), (h_up, w_up))   # :445
            pm = ops.warp_affine_f32(parse[k], dst2src, region) if parse is not None else None   # :478-479
            ops.paste_blend(canvas, faces[k], dst2src, ero, soft, region, parse=pm)    # :400, :432, :481-492
            if draw_box:
                border = box_border(areas[k])                                          # :440
                if border > 0:                                                         # border 0: the band is empty
                    x0, y0, rw, rh = region
                    boxes.append(list(dst2src.reshape(-1)) + [border, x0, y0, x0 + rw, y0 + rh])
        if draw_box:                                                                   # :497 + :502-509 in one launch
            recs = torch.tensor(boxes, dtype=torch.float64).to(self.device) if boxes else None
            out = ops.box_overlay_u8(canvas, recs, (fh, fw))
        else:
            out = ops.f32_to_u8_trunc(canvas)                                          # :497
        return out if return_tensor else out.cpu().numpy()


def box_border(total_face_area):
    """Width of the drawn box band, int(1400 / np.sqrt(total_face_area)) in float32 as numpy evaluates it (:440)."""
    return int(np.float32(1400) / np.sqrt(np.float32(total_face_area)))
