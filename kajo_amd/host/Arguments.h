// Arguments.h -- kajo_render's command line, parsed and checked: what the render and the output stages of Main.cpp take.
#ifndef KAJO_ARGUMENTS_H
#define KAJO_ARGUMENTS_H

#include <cstdint>
#include <string>
#include <vector>

#include "HipScheduler.h"

struct Arguments
{
    hip::Options opt; // (opt.passes 16 and opt.gpus 1 unless given)
    int width = 640, height = 480; // of the rendered frame: --supersample K has multiplied them
    std::string rendererName = "hip", scenePath, podPath;
    bool verbose = false, json = false, threeArg = false, noPreview = false;
    int closeAtEvent = 0;
    // the files written
    std::string out = "out.png", rawOut, hdrOut, noiseMapOut, sampleMapOut, aovPrefix, matteMaskOut, matteIdsOut, denoiseOut, png16Out;
    // what the output stage needs beside the backend's options
    KajoEncodeParams encode16, encode8; // of --png16 and of -o through --dither
    bool dither = false;
    bool encodeView = false; // --encode-view: --png16 and --dither's -o through the float view, at the view's output size
    std::vector<int32_t> matteObjects;
    int denoiseIterations = 5;
    bool whiteBalanceGiven = false;
    double whiteBalanceKelvin = 0, whiteBalanceTint = 0;
    double viewScaleX = 0, viewScaleY = 0; // source pixels per output pixel
    // a stage's options were given (glareGiven: and its parameters change the frame)
    bool toneGiven = false, glareGiven = false, adaptiveGiven = false, noiseGiven = false, meterGiven = false, localGiven = false, viewGiven = false,
         encodeGiven = false, lensGiven = false, gradeGiven = false, matteGiven = false;
};

// The command line into *a, checked before any device is opened. 0, or the exit status with the message on stderr (--help: on stdout).
int parseArguments(int argc, char** argv, Arguments* a);

// the names of KAJO_TRANSFER_* and of KAJO_VIEW_*, indexed by the value
extern const char* const transferNames[4];
extern const char* const viewFilterNames[4];

#endif
