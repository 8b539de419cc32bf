// Stand-in for <FreeImage.h> -- TEST INFRASTRUCTURE ONLY (oracle/_ref).
// Declarations of the names RayTracer::exportImage uses, so that the
// reference's src/rayTracer.cpp compiles where FreeImage is not installed.
// oracle/ref/ref_hot.cpp supplies no-op bodies; exportImage is never called.
#pragma once

typedef unsigned char BYTE;
typedef int BOOL;
struct FIBITMAP;
struct RGBQUAD {
    BYTE rgbBlue, rgbGreen, rgbRed, rgbReserved;
};
enum FREE_IMAGE_FORMAT { FIF_UNKNOWN = -1, FIF_HDR = 26, FIF_EXR = 29 };
enum FREE_IMAGE_TYPE { FIT_UNKNOWN = 0, FIT_BITMAP = 1, FIT_RGBF = 11 };

extern "C" {
void FreeImage_Initialise(BOOL load_local_plugins_only = 0);
void FreeImage_DeInitialise(void);
FREE_IMAGE_FORMAT FreeImage_GetFIFFromFilename(const char *filename);
FIBITMAP *FreeImage_Allocate(int width, int height, int bpp, unsigned red_mask = 0, unsigned green_mask = 0,
                             unsigned blue_mask = 0);
FIBITMAP *FreeImage_AllocateT(FREE_IMAGE_TYPE type, int width, int height, int bpp = 8, unsigned red_mask = 0,
                              unsigned green_mask = 0, unsigned blue_mask = 0);
unsigned FreeImage_GetPitch(FIBITMAP *dib);
BYTE *FreeImage_GetBits(FIBITMAP *dib);
BOOL FreeImage_SetPixelColor(FIBITMAP *dib, unsigned x, unsigned y, RGBQUAD *value);
BOOL FreeImage_Save(FREE_IMAGE_FORMAT fif, FIBITMAP *dib, const char *filename, int flags = 0);
}
